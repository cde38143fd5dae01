/* vgaudio_hip_files/hca_keyed_files.h -- keys for device-resident sets of CRI HCA files (vgaudio_hip/hca_files.h): the key of
 * every file of a set FOUND among the caller's candidates, and the frames of a set of encrypted images read DECRYPTED with
 * per-file key indices that lie in device memory -- each in a fixed number of launches on the caller's stream, whatever the
 * numbers of files and candidates.  encrypted images -> vga_hca_find_keys_device_v -> vga_hca_read_keyed_device_v ->
 * vga_hca_decode_device_v never leaves HBM, and nothing in the chain returns a value to the host or synchronises
 * (HcaReader.cs:39-49 and :238-252, EncryptionKey ?? FindKey; CriHcaEncryption.cs:34-88; for a whole folder, Batch.cs).
 *
 * The calls work on the vga_hca_files objects of vga_hca_files_create_from_infos, created WITHOUT keys of their own
 * (ntables == 0); the layout of images and frames, the alignment rules and everything vga_hca_read_device_v promises are
 * hca_files.h's.  A file's ENCRYPTION TYPE is its vga_hca_file_info.encryption_type.
 *
 * TABLES.  d_tables: decryption tables of 256 bytes each in DEVICE memory, at any byte: what vga_hca_key_tables gives,
 * uploaded by the caller once.  The candidates of a search are d_tables[0 .. nkeys), tried in that order.
 *
 * FIND   d_key_index_out[f] (always written, for every file) and d_status[f] (when given, for every file):
 *   type 56       what vga_hca_find_key_device returns for the file's frames as they lie in the image, over the same
 *                 candidates: the first candidate under which the up to ten frames from the first non-empty one unpack
 *                 (non-empty: a non-zero byte in [2, frame_size - 2); frame 0 when every frame is empty).  A file of no
 *                 frames: index 0 when nkeys > 0.  No candidate passes, or nkeys == 0: index -1, status 1 ("Cannot find key
 *                 to decrypt HCA file.").  A candidate that meets a wrong sync word before its first unpack failure, no
 *                 earlier candidate having won: index -1, status 2 (the per-file call's VGA_ERR_INVALID_DATA, "Invalid
 *                 frame header").  Otherwise status 0.
 *   type 1        type1_index as given (the caller's place for the type-1 table in the tables of the READ; -1 is allowed);
 *                 the search never reads that table.  Status 0.
 *   anything else -1, status 0 (HcaReader.FindKey returns null).
 * Nothing else is written outside the workspace, whose contents on entry do not matter.  The index tensor goes straight into
 * vga_hca_read_keyed_device_v on the same stream.
 *
 * READ   d_key_index[f] in [0, ntables): file f's frames are what vga_hca_read_device followed by vga_hca_crypt_device with
 * d_tables[d_key_index[f]] leaves; negative: vga_hca_read_device_v's, unkeyed; >= ntables: moved unkeyed, status 1.
 * d_key_index == NULL: table 0 for every file.  d_status (when given) is written for every file: 0 or 1 (one more launch of
 * nfiles threads).  Bad-CRC counts (ADDED to d_bad_crc) and the zero bytes up to the next multiple of 4 are as in
 * vga_hca_read_device_v.
 *
 * WHICH KERNELS.  The read runs the kernels of hca_files.h: the table index is a value every work item reads, from the set's
 * own table (keys given at create) or from d_key_index.  Files of up to 4096-byte frames are deciphered inside the copy in LDS
 * (the span form: every frame byte crosses HBM once each way), larger frames take the general form, and
 * vga_hca_files_force_general_this_thread(1) applies.  The search is four launches: a wave per file finds the first tested
 * frame and the number of tested frames, reading only the frames in front of it; a wave per (file, 64 candidates) stages the
 * file's first tested frame and the 64 tables in LDS and every lane walks the frame under its candidate -- wrong keys mostly
 * end there; the candidates that passed walk the later frames, a lane per (candidate, frame); a wave per file puts the
 * outcomes back in candidate order.  A first tested frame of more than 2048 bytes, and later frames of more than 9216 bytes
 * together, are not staged: the same walk reads them from global memory.  Every (file, candidate) has its own outcome byte
 * in the workspace, so the result does not depend on scheduling.
 *
 * REFUSED before anything is launched, the message naming the call.  VGA_ERR_ARGUMENT: whatever hca_files.h refuses for a read
 * (d_images not 16-byte, d_frames not 4-byte aligned, a required buffer missing), a null d_tables with candidates or tables to
 * read, ntables <= 0 for the read, nkeys < 0, type1_index < -1, a null d_key_index_out, a workspace that is null, too small
 * or not int-aligned, a type-56 file whose header vga_hca_find_key_device refuses.  VGA_ERR_INVALID_OP: a set made for
 * writing, and a set created with keys of its own (two sources of keys in one call are ambiguous).  nfiles == 0 returns 0 and
 * launches nothing.  All calls run on the caller's stream and never synchronise it; they allocate nothing and copy nothing
 * from host memory; there is no memset.
 *
 * LEFT OUT: a keyed WRITE with device-chosen keys (the header's ciph chunk and id bits are built at create from the key: the
 * writer's key is a create-time fact, vga_hca_files_create); the `crackhca` statistics over a set; host-pointer forms; moving
 * vga_hca_find_key_device onto the new kernels (that changes an existing call's launches and belongs to a change of its
 * own). */
#ifndef VGAUDIO_HIP_FILES_HCA_KEYED_FILES_H
#define VGAUDIO_HIP_FILES_HCA_KEYED_FILES_H

#include "../vgaudio_hip/hca_files.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the workspace of a search with that many candidates on this set; 0 for an empty set, and for a set made for
 * writing or a negative count (the call itself says why) */
size_t vga_hca_find_keys_workspace_bytes(const vga_hca_files *s, int nkeys);
int vga_hca_find_keys_device_v(const vga_hca_files *s, const uint8_t *d_images, const uint8_t *d_tables, int nkeys, int type1_index,
                               int *d_key_index_out, int *d_status /* nfiles or NULL */, void *d_workspace, size_t workspace_bytes,
                               void *stream);
int vga_hca_read_keyed_device_v(const vga_hca_files *s, const uint8_t *d_images, const uint8_t *d_tables, int ntables,
                                const int *d_key_index, uint8_t *d_frames, int *d_bad_crc /* nfiles or NULL */,
                                int *d_status /* nfiles or NULL */, void *stream);

/* ---- hook of this feature (tests and tools), host only: the work items of the search's two test launches on a set of such
 * infos with nkeys candidates, in launch order.  Every (type-56 file, candidate) lies in exactly one item; other files have
 * none.  items_out may be NULL (the count alone); more than `capacity` items is VGA_ERR_ARGUMENT with the count in
 * *count_out. */
typedef struct { int file, first_key, key_count; } vga_hca_find_keys_item;
int vga_hca_find_keys_items_for(const vga_hca_file_info *const *infos, int nfiles, int nkeys, vga_hca_find_keys_item *items_out,
                                int64_t capacity, int64_t *count_out);

#ifdef __cplusplus
}
#endif
#endif

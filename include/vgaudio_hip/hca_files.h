/* vgaudio_hip/hca_files.h -- device-resident sets of CRI HCA FILES of different shapes: the image of every file of a set,
 * written and read, in one fixed set of launches per call, with the key substitution and the frame CRC-16 done on the copy.
 * The consumer of the frames hca_ragged.h leaves: WAV set -> vga_hca_encode_device_v -> vga_hca_write_device_v never leaves
 * HBM and issues no launch per file or per key (HcaWriter for a whole folder, VGAudio.Cli/Batch.cs), and neither does
 * images -> vga_hca_read_device_v.  The fourth codec family with file sets (gc_files.h, nw_files.h, adx_files.h).
 *
 * It lives next to adx_files.h and outside the directory listing the older test files enumerate; the same disciplines are
 * applied to THIS header by tests/test_hca_files_host.py (exports, argument counts, the layout against a model, the work
 * items' tiling, the form every file takes, every refusal, and that the GPU file's table of cases names every function
 * declared here) and tests/test_gpu_hca_files.py (junk-filled buffers larger than needed, poison mode, a busy caller
 * stream, two streams at once).  The hooks of this feature are declared here too, at the end.
 *
 * A SET is nfiles files (vga_hca_file: the arguments of vga_hca_write_device for that file -- its vga_hca_info, comment,
 * volume, encryption_type and encrypted_ids -- and `key`, an index into the set's substitution tables or -1).  The tables
 * are `ntables` tables of 256 bytes in host memory, copied at create: what vga_hca_key_tables gives (the encryption table
 * for a set that writes, the decryption table for one that reads), one per key in use, so files of several keys share a
 * call.  The set is NOT limited to one shape class: channel counts, frame sizes and header sizes are per file.
 *
 * LAYOUT (vga_hca_files_layout_for computes it on the host, no GPU needed; an object carries the same numbers)
 *   frames  file f's frames lie back to back at d_frames + frame_offsets[f] (bytes), frame_count * frame_size of them.
 *           frame_offsets == NULL: packed as vga_hca_ragged_layout_for packs them -- ascending in file order, each stream
 *           rounded up to 4, 8 bytes of slack behind the last whose content does not matter -- so ONE vga_hca_ragged
 *           object's output is a set's input as it lies.  frame_offsets != NULL (one per file): the caller's offsets,
 *           multiples of 4, streams must not overlap (a stream owns its bytes up to the next multiple of 4);
 *           totals.frame_bytes is then the end of the furthest stream rounded up to 4, plus 8.  That is for sets of several
 *           shape classes: each ragged object's buffer at a base inside one allocation.  A file of no frames takes no room.
 *           d_frames must be 4-byte aligned.
 *   images  image f is hca.header_size + frame_count * frame_size bytes (vga_hca_file_size) at image_offsets[f] of one
 *           buffer of totals.image_bytes.  Packed images are each rounded up to 16 bytes and a guard of 256 bytes follows
 *           the last (nothing writes it).  A set made from parsed headers takes image f from frames_offset to the end of
 *           its frames, at ANY byte offset the caller names (HCA files inside archives are not aligned), or packed as above.
 *           The packed buffers' bases (d_images) must be 16-byte aligned.
 *   Anything less, or a null required buffer, is VGA_ERR_ARGUMENT before anything is launched.  nfiles == 0 is an empty
 *   set: every call returns 0 and launches nothing.
 *
 * WRITE  image f is byte for byte what this sequence writes for that file alone: vga_hca_crypt_device with the file's
 * table if key >= 0, then vga_hca_write_device with the file's comment, volume, encryption_type and encrypted_ids
 * (HcaWriter.cs:39-45, :57-82, :173-179).  d_frames is NOT modified: the reference encrypts the format in place, the set
 * encrypts the copy.  Headers are built on the host at create by the code behind vga_hca_file_header, CRC included, and kept
 * in device memory with the set's tables.  key == -1: the frames are copied as they are, a bad CRC included.  key >= 0: the
 * first frame_size - 2 bytes of every frame go through the table and the CRC-16 is refreshed (CriHcaEncryption.CryptFrame),
 * also when the table is the identity.  A keyed file's frames may be 2 .. 65535 bytes (vga_hca_crypt_device itself stops
 * at 4096).  A fixed number of launches whatever nfiles is (headers, span items, general items), no memset:
 * every byte of every image is written, and no byte between two images, in a guard or of d_frames is.
 * READ   file f's frames arrive as vga_hca_read_device delivers them, followed by vga_hca_crypt_device with the file's
 * table if it has a key (HcaReader.cs:41-46, :123-138).  The CRC-16 of each frame AS STORED in the image is compared with
 * its last two bytes and the mismatches are ADDED to d_bad_crc[f] (one int per file; the caller zeroes the array, as with
 * d_status in hca_ragged.h); bad frames are kept.  d_bad_crc == NULL: no counts, and for a file without a key no CRC is
 * computed at all.  Behind a stream's last frame only the bytes up to the next multiple of 4 are written, as zeros; nothing
 * else is: not the slack, not the gaps between explicit offsets, not d_images.
 *
 * REFUSED AT CREATE AND LAYOUT, before anything is launched, the message naming the file ("file <f>: " in front of the
 * per-file message) with the per-file call's own code, because the check IS that call's code: whatever vga_hca_file_size
 * ("HCA file size out of range", VGA_ERR_OUT_OF_RANGE), vga_hca_file_header (a header size outside 8..0x7FFF
 * VGA_ERR_OUT_OF_RANGE, chunks that do not fit VGA_ERR_INVALID_OP) or vga_hca_read_device ("info does not describe an HCA
 * file", VGA_ERR_ARGUMENT) refuse.  Of the set itself: a key outside -1 .. ntables-1, ntables > 0 with null tables (or
 * ntables < 0), a keyed file with frames outside 2 .. 65535 bytes, a frame offset that is negative or no multiple of 4,
 * overlapping streams, a null info, a negative image offset VGA_ERR_ARGUMENT; totals past 2^62 bytes VGA_ERR_OUT_OF_RANGE.
 *
 * A set made for writing refuses the read call and the other way round with VGA_ERR_INVALID_OP.
 *
 * WHICH KERNELS.  The SPAN form serves frames of up to 4096 bytes: a workgroup takes a span of whole frames of one file (at
 * most 16 KiB), loads it into LDS with aligned 16-byte loads whatever the source's alignment is, computes on the copy the
 * stored-bytes CRC (read side, when asked), the substitution through the file's table in LDS and the refreshed CRC, and
 * stores it with aligned 16-byte stores at the destination's own alignment; lead and tail bytes go singly.  Every frame byte
 * crosses HBM once each way.  Every other frame size takes the GENERAL form: a workgroup per item of whole frames, byte by
 * byte in global memory.  Header items copy the prebuilt headers.  vga_hca_files_stats says how many files and items take
 * which form.
 *
 * All calls run on the caller's stream and never synchronise it; they need no workspace; the library allocates nothing per
 * call.  The object keeps its tables in the memory of the device that was current at create, is immutable and serves any
 * number of calls, concurrent calls on different streams included.
 *
 * FindKey inside a set, and a read whose keys are indices in device memory, are vgaudio_hip_files/hca_keyed_files.h's
 * (vga_hca_find_keys_device_v, vga_hca_read_keyed_device_v, on the objects of vga_hca_files_create_from_infos).
 * LEFT OUT: host-pointer forms of the _v calls; moving the per-file vga_hca_write_device,
 * vga_hca_read_device and vga_hca_crypt_device onto the new body (that changes existing calls' launches and belongs to a
 * change of its own). */
#ifndef VGAUDIO_HIP_HCA_FILES_H
#define VGAUDIO_HIP_HCA_FILES_H

#include "hca_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    vga_hca_info hca;
    const char *comment;
    float volume;
    int encryption_type;
    int encrypted_ids;
    int key;
} vga_hca_file;                                    /* the arguments of vga_hca_write_device, per file; key: index into the set's tables, -1 = none */
typedef struct { int files; int64_t total_frames, frame_bytes, image_bytes; } vga_hca_files_totals;   /* slack and guards included */
typedef struct vga_hca_files vga_hca_files;

/* host only, needs no GPU.  frame_offsets: one per file, or NULL for packed streams.  The outputs have nfiles entries; any may
 * be NULL, but not all of them. */
int  vga_hca_files_layout_for(const vga_hca_file *files, int nfiles, const int64_t *frame_offsets, int64_t *frame_offsets_out,
                              int64_t *image_offsets_out, vga_hca_files_totals *totals_out);
/* the same checks, then the tables in the current device's memory.  tables: ntables x 256 bytes, host memory */
int  vga_hca_files_create(const vga_hca_file *files, int nfiles, const int64_t *frame_offsets, const uint8_t *tables, int ntables,
                          vga_hca_files **out);
/* a set for READING, from what vga_hca_parse returned for every file.  Image f is at image_offsets[f] (any byte), or packed as
 * the writer packs; keys: one table index per file (-1 = none), or NULL for no keys at all. */
int  vga_hca_files_create_from_infos(const vga_hca_file_info *const *infos, int nfiles, const int64_t *image_offsets /* NULL: packed */,
                                     const int *keys /* nfiles or NULL */, const uint8_t *tables, int ntables,
                                     const int64_t *frame_offsets /* NULL: packed */, vga_hca_files **out);
void vga_hca_files_destroy(vga_hca_files *s);
int  vga_hca_files_totals_of(const vga_hca_files *s, vga_hca_files_totals *out);
int  vga_hca_files_offsets(const vga_hca_files *s, int64_t *frame_offsets_out, int64_t *image_offsets_out);

int  vga_hca_write_device_v(const vga_hca_files *s, const uint8_t *d_frames, uint8_t *d_images, void *stream);
int  vga_hca_read_device_v(const vga_hca_files *s, const uint8_t *d_images, uint8_t *d_frames, int *d_bad_crc /* nfiles or NULL */,
                           void *stream);

/* ---- hooks of this feature (tests and tools)
 * The work items of a set, host only: what the kernels of a call are launched over, in launch order.  begin / end: the bytes
 * the item writes, counted from the start of the file's image (write) or of the file's stream (read; the last item of a
 * stream ends at the stream's length rounded up to 4).  HEADER items exist in a set for writing only, one per file.
 * first_frame / frames: the whole frames a SPAN or GENERAL item moves.  general != 0: the items of a call under
 * vga_hca_files_force_general_this_thread(1).  items_out may be NULL (the count alone); more than `capacity` items is
 * VGA_ERR_ARGUMENT with the count in *count_out. */
#define VGA_HCA_FILES_HEADER 0
#define VGA_HCA_FILES_SPAN 1
#define VGA_HCA_FILES_GENERAL 2
typedef struct { int form, file, first_frame, frames; int64_t begin, end; } vga_hca_files_item;
int  vga_hca_files_write_items_for(const vga_hca_file *files, int nfiles, const int64_t *frame_offsets, int general,
                                   vga_hca_files_item *items_out, int64_t capacity, int64_t *count_out);
int  vga_hca_files_read_items_for(const vga_hca_file_info *const *infos, int nfiles, const int64_t *image_offsets,
                                  const int64_t *frame_offsets, int general, vga_hca_files_item *items_out, int64_t capacity,
                                  int64_t *count_out);
/* out[0..3]: files in the span form, files in the general form (files of no frame bytes count in neither), span items,
 * general items -- of a call made by this thread now (the force hook applies) */
int  vga_hca_files_stats(const vga_hca_files *s, int64_t *out /*[4]*/);
/* per thread: the _v calls of this thread take the general form for every file.  Returns the previous value. */
int  vga_hca_files_force_general_this_thread(int on);

#ifdef __cplusplus
}
#endif
#endif

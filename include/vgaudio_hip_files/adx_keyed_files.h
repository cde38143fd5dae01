/* vgaudio_hip_files/adx_keyed_files.h -- keyed encryption for device-resident sets of CRI ADX files (vgaudio_hip/adx_files.h):
 * the images of a set written ENCRYPTED, the rows of a set of encrypted images read DECRYPTED, and the key of every file of a
 * set FOUND among the caller's candidates -- each in a fixed number of launches on the caller's stream, whatever the number
 * of files.  WAV set -> vga_adx_encode_device_v -> vga_adx_write_keyed_device_v never leaves HBM; neither does encrypted
 * images -> vga_adx_find_keys_device_v -> vga_adx_read_keyed_device_v -> vga_adx_decode_device_v, and nothing in either chain
 * returns a value to the host or synchronises (AdxWriter.cs:123-131; AdxReader.cs:31, EncryptionKey ?? FindKey(structure),
 * and :40-43, for a whole folder).
 *
 * The calls work on the vga_adx_files objects of vga_adx_files_create (write) and vga_adx_files_create_from_infos (read,
 * find); the layout of rows and images, the alignment rules and everything the unkeyed calls promise are adx_files.h's.
 * A file's ENCRYPTION TYPE is the file's own: params.encryption_type for a set made for writing (the header byte
 * AdxWriter.cs:92 writes), info.revision for a set made from parsed headers.
 *
 * THE CIPHER (CriAdxEncryption.cs:16-41).  A slot is frame * channel_count + channel: in an image simply the frame's position
 * in the audio.  The 15-bit state x -> (x * mult + inc) & 0x7fff advances once per slot, empty frames included; a frame
 * that holds a non-zero byte (the whole frame, looked at before it is changed) has its first byte XORed with the state's
 * high byte and its second with the low byte.  Slot 0 uses the caller's raw, unmasked seed.  Type 9 then masks the first
 * byte with 0x1f; every other type value only XORs, as vga_adx_crypt_device does.  vga_adx_crypt_device and
 * vga_adx_find_key_device define the result of these calls for every type value.
 *
 * KEYS.  d_keys: nkeys vga_adx_key in DEVICE memory (12 bytes each, at any int boundary).  d_key_index: one int per file in
 * device memory, or NULL = key 0 for every file; index < 0: the file is moved unkeyed.  d_status: one int per file or NULL;
 * the call writes EVERY entry: 0, or 1 = the index is >= nkeys and the file was moved unkeyed (one more launch of nfiles
 * threads, made only when d_status is given).
 *
 * WRITE  For a file with a valid key index the image is byte for byte what vga_adx_crypt_device on a copy of its rows
 * followed by vga_adx_write_device writes, with that key, the file's type and the file's frame size; for every other file
 * what vga_adx_write_device_v writes.  d_audio is const and stays as it was.  No memset, no byte written between images or
 * into guards, and the header overrun, truncation and footer quirks of adx_files.h hold.
 * READ   Row c of a keyed file is what vga_adx_read_device then vga_adx_crypt_device leave, with encryption_type = revision
 * (also when the revision is 0 and the caller names a key, AdxReader.cs:31,40-43); every other file's rows are
 * vga_adx_read_device_v's.
 * FIND   Candidates: d_keys[0 .. nkeys8) are tried on files of revision 8, d_keys[nkeys8 .. nkeys8 + nkeys9) on every other
 * non-zero revision (CriAdxEncryption.cs:46); revision 0 gives -1 (AdxReader.cs:128), and so does an empty sub-list.
 * d_key_index_out[f] is an index INTO d_keys: what vga_adx_find_key_device returns for file f's rows over the sub-list of its
 * revision, plus that sub-list's base, or -1 -- the first candidate TestKey (CriAdxEncryption.cs:79-94) passes over all
 * frame_count * channel_count scales, a scale of 0 agreeing with every key.  The array goes straight into
 * vga_adx_read_keyed_device_v on the same stream.  The workspace's contents on entry do not matter.
 *
 * WHICH KERNELS.  Files in the SPAN form (18-byte frames, at most 113 channels, rows at multiples of 16) are ciphered inside
 * the copy: the span kernels of adx_files.h hold whole frames in LDS between load and store, one thread per frame tests
 * emptiness there and XORs the two bytes, so every byte still crosses HBM once each way.  A thread jumps the LCG once to its
 * first slot and steps by a stride of 256 slots.  Files in the GENERAL form get a cipher pass of their own over the call's
 * output (the frames in the image for a write, the rows for a read) over (file, chunk of 2048 slots) items cut at create:
 * one launch more than the unkeyed call.  vga_adx_files_force_general_this_thread(1) sends keyed calls down this path too.
 * The search is three launches: one "still possible" bit per (file, candidate) is set in the workspace; a workgroup per
 * (file, span of 1024 slots) reads the span's scales out of the image once and, 64 candidates x 4 quarters of the span at a
 * time, walks the LCG of every candidate still possible along them, clearing the bit of one that fails (bits are only ever
 * cleared, and read in the next launch: the result does not depend on scheduling); the lowest surviving bit of a file's
 * sub-list is its answer.
 *
 * REFUSED before anything is launched, VGA_ERR_ARGUMENT: what adx_files.h refuses (d_audio / d_images not 16-byte aligned, a
 * required buffer missing), a null d_keys with candidates to read, nkeys <= 0 for the two keyed calls, a negative count, a
 * null d_key_index_out, a workspace that is null or too small, a set with a file of 1-byte frames (no scale to cipher).  A set
 * made for writing refuses the read and find calls with VGA_ERR_INVALID_OP, and the other way round.  nfiles == 0 returns 0
 * and launches nothing.  All three run on the caller's stream and never synchronise it; they allocate nothing and copy
 * nothing from host memory.
 *
 * HCA FindKey inside a set is hca_keyed_files.h's, next to this header.
 * LEFT OUT: the `crackadx` brute force (vga_adx_guess_keys) over a set; host-pointer forms of these calls. */
#ifndef VGAUDIO_HIP_FILES_ADX_KEYED_FILES_H
#define VGAUDIO_HIP_FILES_ADX_KEYED_FILES_H

#include "../vgaudio_hip/adx_files.h"

#ifdef __cplusplus
extern "C" {
#endif

int vga_adx_write_keyed_device_v(const vga_adx_files *s, const uint8_t *d_audio, const int16_t *d_history,
                                 const vga_adx_key *d_keys, int nkeys, const int *d_key_index,
                                 uint8_t *d_images, int *d_status, void *stream);
int vga_adx_read_keyed_device_v(const vga_adx_files *s, const uint8_t *d_images,
                                const vga_adx_key *d_keys, int nkeys, const int *d_key_index,
                                uint8_t *d_audio, int16_t *d_history_out, int *d_status, void *stream);

/* bytes of the workspace of a search with that many candidates on this set; 0 for an empty set, and for a set not made for
 * reading or negative counts (the call itself says why) */
size_t vga_adx_find_keys_workspace_bytes(const vga_adx_files *s, int nkeys8, int nkeys9);
int vga_adx_find_keys_device_v(const vga_adx_files *s, const uint8_t *d_images, const vga_adx_key *d_keys,
                               int nkeys8, int nkeys9, int *d_key_index_out,
                               void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- hook of this feature (tests and tools), host only: the work items of the search's scan launch on a set of such
 * infos, in launch order.  Every slot of every file lies in exactly one item.  items_out may be NULL (the count alone); more
 * than `capacity` items is VGA_ERR_ARGUMENT with the count in *count_out. */
typedef struct { int file, first_slot, slot_count; } vga_adx_find_keys_item;
int vga_adx_find_keys_items_for(const vga_adx_file_info *const *infos, int nfiles, const int64_t *image_offsets,
                                vga_adx_find_keys_item *items_out, int64_t capacity, int64_t *count_out);

#ifdef __cplusplus
}
#endif
#endif

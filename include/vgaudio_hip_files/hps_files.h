/* vgaudio_hip_files/hps_files.h -- device-resident sets of HPS FILES of different shapes: the HPS image of every file of a set,
 * written and read, in one set of launches per call.  A consumer of the rows gc_files_aligned.h leaves: WAV set ->
 * vga_gcadpcm_coefs_device_v -> vga_gcadpcm_encode_device_v -> vga_gcadpcm_align_channels_device_v -> vga_hps_write_device_v
 * never leaves HBM and issues no launch per file, and neither does images -> vga_hps_read_device_v ->
 * vga_gcadpcm_decode_device_v.  The scaffolding is nw_files.h's; idsp_files.h is this header's twin.
 *
 * It lives in the directory of wave_files.h, outside the listings the older test files enumerate; the same disciplines are
 * applied to THIS header by tests/test_hps_files_host.py (exports, argument counts, the layout against a model, the regions
 * the kernels write, every refusal, and that the GPU file's table of cases names every function declared here) and
 * tests/test_gpu_hps_files.py (junk-filled buffers larger than needed, poison mode, a busy caller stream, two streams at
 * once).  The hooks of this feature are declared here too, at the end.
 *
 * A SET is nfiles files (vga_hps_file: channel count, sample rate, sample count and the format's loop, before the writer
 * aligns it).  File f's vga_hps_params are the file's numbers, and everything about file f is what vga_hps_layout_for and
 * vga_hps_block_map say for them: an HPS image is NOT a header plus one interleave but a header and a chain of blocks of at
 * most 64 KiB, each with a header of its own (every channel's pred/scale byte, hist1 and hist2 at the block's first sample).
 *
 * LAYOUT (vga_hps_files_layout_for computes it on the host, no GPU needed; an object carries the same numbers)
 *   inputs  lie exactly as gc_files_aligned.h leaves its OUTPUT: the channels of file f are rows first_channel[f] ..
 *           first_channel[f] + channels - 1 of a GC ragged batch over each file's sample_count_aligned, from
 *           vga_gcadpcm_channel_layout_for(layout.channel) (vga_hps_files_ragged; rows rounded to 16 bytes, a guard of 256
 *           bytes behind the last); a row's ADPCM is layout.channel_adpcm_bytes bytes.  totals.adpcm_bytes / pcm_samples are
 *           the batch's sizes, guards included.  Per-channel arrays (d_coefs: 16 shorts, d_gain: 1, d_start_context: 3) are
 *           indexed by row.  d_pcm is the aligned set's d_pcm_out in the same ragged layout: the block headers' hist1 / hist2
 *           are Pcm[start_sample - 1 / - 2] of the row; NULL gives zeros, as the per-file call does.
 *           vga_hps_files_gc_files fills the vga_gc_file array (channel = layout.channel: the loop alignment multiple is
 *           ByteCountToSampleCount(GetNextMultiple(0x10000 / channels, 0x20)) and differs with the channel count) that
 *           vga_gc_aligned_create takes.  The set does not own or need the aligned object.
 *   images  File f's image is layout.file_size bytes at image_offsets[f] of one buffer of totals.image_bytes; offsets are
 *           rounded up to 16 bytes and a guard of 256 bytes follows the last image (nothing writes it).  The blocks of file f
 *           are entries first_block[f] .. of the set's block table, totals.blocks in all.
 *   EVERY HPS image size, header size, block offset, padded channel size and byte_in_index is a multiple of 0x20 (the
 *   writer rounds each to 0x20, and only a file's LAST block may hold a number of nibbles that is no multiple of 0x40), so rows
 *   and images move as 16-byte vectors throughout; tests/test_hps_files_host.py holds this over the test sets.
 *   d_adpcm, d_pcm and d_images must be 16-byte aligned.  Anything less, or a null required buffer, is VGA_ERR_ARGUMENT before
 *   anything is launched.  nfiles == 0 is an empty set: every call returns 0 and launches nothing.
 *
 * REFUSED AT CREATE AND LAYOUT, the message naming the file ("file <f>: " in front of the per-file message), with the
 * per-file call's own code, because the check IS vga_hps_layout_for's code (gc_stream_host.hpp): no channel VGA_ERR_ARGUMENT;
 * more than 255 channels, or 3, 7, 11, ... channels (nch % 4 == 3) VGA_ERR_INVALID_OP; a file without a block, loop points
 * WithLoop rejects, a file past 2 GiB VGA_ERR_OUT_OF_RANGE; a block whose hist index lies at or past the PCM row
 * VGA_ERR_OUT_OF_RANGE (vga_hps_write_device's check with pcm_len = the row's sample_count_aligned; a block map over rows of
 * that length never trips it, it guards the tables).  The set's own limits: more than 2^31 rows, or blocks plus files, or
 * work items VGA_ERR_ARGUMENT; images of more than 2^62 bytes VGA_ERR_OUT_OF_RANGE.
 * KNOWN LIMIT, inherited from vga_hps_layout_for: a file of more than about 1.88e9 samples (2^31 nibbles) is not refused but
 * ends the process, as the nibble count wraps in int before the 2 GiB check is reached; "a file past 2 GiB" above holds
 * below that count.  No HPS file can be that long (2 GiB of image is 3.7e9 nibbles over all channels); keep sample counts
 * below it.
 *
 * A set made for writing refuses the read call and the other way round with VGA_ERR_INVALID_OP.
 *
 * LAUNCHES.  A write is TWO launches whatever nfiles is: (1) the headers, one workgroup per file and one per block -- a
 * file's stream header and channel infos with all zero padding up to header_size, a block's header (WrittenSize, EndNibble,
 * NextOffset, then per channel the pred/scale byte at start_sample / 14 * 8 of the row, hist1, hist2) with all zero padding
 * up to block_header_size; (2) the block bodies over (block, chunk) work items cut on the host so that none lies outside its
 * image and the grid is exactly the item count, the zero padding of a channel's last partial 0x20 line written by the item
 * that owns it.  A read is at most TWO: the parsed per-channel arrays (only if one is asked for), then one gather over
 * (block, channel, chunk) items.  A launch without items is not made.  There is no memset: every byte of every image is
 * written exactly once by these kernels, and no byte between two images, behind the last image or in the guard is.
 * vga_hps_files_stats reports the launches of the last call.
 *
 * READ SETS take images at the caller's offsets: int64_t, ANY byte offset that is not negative (HPS files inside archives do
 * not start aligned; images that overlap are the caller's business, they are only read), or packed as the writer packs.  A
 * block whose audio address (image offset + audio_offset), channel stride (size / channels) and out_offset are multiples of
 * 16 moves 16-byte vectors, its ragged end bytes; any other block -- foreign geometry -- takes the GENERAL form of the gather,
 * byte by byte.  It is not refused: whatever vga_hps_read_device reads, the set reads.
 *
 * All calls run on the caller's stream and never synchronise it; they need no workspace; the library allocates nothing per
 * call and writes nothing outside an image (write) or a row and a per-channel array (read): not the rounding gaps, not
 * the guards.  The object keeps its tables (the block table goes up once, at create) in the memory of the device that was
 * current at create, is immutable and serves any number of calls, concurrent calls on different streams included.
 *
 * LEFT OUT: host-pointer forms of the _v calls; a custom MaxBlockSize (the reference's writer has none either). */
#ifndef VGAUDIO_HIP_FILES_HPS_FILES_H
#define VGAUDIO_HIP_FILES_HPS_FILES_H

#include "../vgaudio_hip/gc_files_aligned.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int channels;                          /* 1 .. VGA_GC_CONTAINER_MAX_CHANNELS, not 3, 7, 11, ... */
    int sample_rate;
    int sample_count;                      /* the format's UnalignedSampleCount */
    int looping, loop_start, loop_end;     /* the format's loop, before the writer aligns it */
} vga_hps_file;
typedef struct {
    int files, channels;
    int64_t pcm_samples, adpcm_bytes;      /* = the GC ragged object's over sample_count_aligned, guards included */
    int64_t image_bytes;                   /* packed images, guard included */
    int64_t blocks;                        /* entries of the set's block table (32 bytes each) */
} vga_hps_files_totals;
typedef struct vga_hps_files vga_hps_files;

/* host only, needs no GPU.  first_channel_out / image_offsets_out / first_block_out: nfiles entries; any output may be NULL,
 * but not all of them. */
int  vga_hps_files_layout_for(const vga_hps_file *files, int nfiles, int *first_channel_out, int64_t *image_offsets_out,
                              int64_t *first_block_out, vga_hps_files_totals *totals_out);
/* the same checks, then the tables in the current device's memory */
int  vga_hps_files_create(const vga_hps_file *files, int nfiles, vga_hps_files **out);
/* a set for READING, from what vga_hps_parse returned for every file: infos[f] and blocks_per_file[f] (infos[f]->block_count
 * entries).  The rows are over each header's sample_count (info->adpcm_bytes bytes); image f reaches to the end of its last
 * block (audio_offset + size, which is the file's end where HpsWriter wrote it) and lies at image_offsets[f], or packed as the
 * writer packs.  The object uploads the block table and
 * the parsed coefficients, gains and contexts once.  An info or a block vga_hps_read_device refuses (or an info whose
 * adpcm_bytes is not its sample count's, or a block at a negative offset) is VGA_ERR_ARGUMENT, naming the file. */
int  vga_hps_files_create_from_infos(const vga_hps_info *const *infos, const vga_hps_block_info *const *blocks_per_file,
                                     int nfiles, const int64_t *image_offsets /* NULL: packed as the writer packs */,
                                     vga_hps_files **out);
void vga_hps_files_destroy(vga_hps_files *s);
int  vga_hps_files_totals_of(const vga_hps_files *s, vga_hps_files_totals *out);
int  vga_hps_files_offsets(const vga_hps_files *s, int *first_channel_out, int64_t *image_offsets_out, int64_t *first_block_out);
/* out: totals.files entries, {channels, sample_rate, layout.channel} of every file: what vga_gc_aligned_create takes.  A
 * set for reading has no writer configuration: VGA_ERR_INVALID_OP. */
int  vga_hps_files_gc_files(const vga_hps_files *s, vga_gc_file *out);
/* borrowed; lives as long as s.  NULL for an empty set made where there is no device. */
const vga_gcadpcm_ragged *vga_hps_files_ragged(const vga_hps_files *s);

/* HpsWriter.cs for every file: image f is byte for byte what vga_hps_write_device writes for that file alone from rows of
 * layout.channel_adpcm_bytes bytes, the NULL-pointer defaults of that call included (d_gain NULL: 0; d_start_context NULL:
 * (the row's first byte, 0, 0); d_pcm NULL: hist1 = hist2 = 0). */
int  vga_hps_write_device_v(const vga_hps_files *s, const uint8_t *d_adpcm, const int16_t *d_coefs, const int16_t *d_gain,
                            const int16_t *d_start_context, const int16_t *d_pcm, uint8_t *d_images, void *stream);
/* The bytes vga_hps_read_device delivers for every file, into the rows of the ragged layout (nothing is written behind a
 * row's end); the per-channel outputs that are not NULL get what the infos hold, so vga_gcadpcm_decode_device_v on
 * vga_hps_files_ragged(s) can follow without a host round trip.  The set is one from vga_hps_files_create_from_infos. */
int  vga_hps_read_device_v(const vga_hps_files *s, const uint8_t *d_images, uint8_t *d_adpcm, int16_t *d_coefs,
                           int16_t *d_gain, int16_t *d_start_context, int16_t *d_loop_context, void *stream);

/* ---- hooks of this feature (tests and tools)
 * The regions a call's kernels write, host only (no GPU), computed from the work tables a set of these arguments holds, in
 * launch order.  kernel: VGA_HPS_FILES_HEADER (write: one per file), VGA_HPS_FILES_BLOCK_HEADER (write: one per block) or
 * VGA_HPS_FILES_AUDIO (one per work item).  index: the file (write) or the row (read).  begin / end: the bytes written,
 * counted from the start of the file's image (write) or of the row (read).  granule: 16 or 1, the vector the item moves (0:
 * the headers).  regions_out may be NULL (the count alone); more than `capacity` regions is VGA_ERR_ARGUMENT with the count
 * in *count_out. */
#define VGA_HPS_FILES_HEADER 0
#define VGA_HPS_FILES_BLOCK_HEADER 1
#define VGA_HPS_FILES_AUDIO 2
typedef struct { int kernel, index, granule; int64_t begin, end; } vga_hps_files_region;
int  vga_hps_files_write_regions_for(const vga_hps_file *files, int nfiles, vga_hps_files_region *regions_out, int64_t capacity,
                                     int64_t *count_out);
int  vga_hps_files_read_regions_for(const vga_hps_info *const *infos, const vga_hps_block_info *const *blocks_per_file, int nfiles,
                                    const int64_t *image_offsets, vga_hps_files_region *regions_out, int64_t capacity,
                                    int64_t *count_out);
/* out[0..3]: the audio work items, the entries of the block table, the bytes of the object's device tables, the kernels the
 * last _v call of THIS thread on any vga_hps_files launched (0 after a refused call or one on an empty set) */
int  vga_hps_files_stats(const vga_hps_files *s, int64_t *out /*[4]*/);

#ifdef __cplusplus
}
#endif
#endif

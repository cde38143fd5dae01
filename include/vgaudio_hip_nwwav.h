/* vgaudio_hip_nwwav.h -- NintendoWare wave files (BRWAV, BCWAV, BFWAV) and stream prefetch files (BCSTP, BFSTP), one
 * at a time on the host and whole sound banks at once on the device.
 *
 * The reference reads them with Containers/NintendoWare/BrwavReader.cs (RWAV) and with the WaveInfoBlock /
 * WaveDataBlock / StreamPrefetchDataBlock branches of BCFstmReader.cs (CWAV, FWAV, CSTP, FSTP); Common.ToAudioStream
 * turns each into a GcAdpcmFormat, Pcm16Format or Pcm8SignedFormat.  It writes none of them, and neither does this
 * library.  vga_nwstm_parse keeps refusing these files: the calls here are a family of their own.
 */
#ifndef VGAUDIO_HIP_NWWAV_H
#define VGAUDIO_HIP_NWWAV_H

#include "vgaudio_hip_pcm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VGA_NWWAV_RWAV 0 /* BrwavReader.cs */
#define VGA_NWWAV_CWAV 1 /* BCFstmReader.cs, WaveInfoBlock + WaveDataBlock */
#define VGA_NWWAV_FWAV 2
#define VGA_NWWAV_CSTP 3 /* BCFstmReader.cs, StreamInfoBlock + StreamPrefetchDataBlock */
#define VGA_NWWAV_FSTP 4

typedef struct {
    int kind;                            /* VGA_NWWAV_*, by the magic */
    int endianness;                      /* VGA_NW_LITTLE_ENDIAN / VGA_NW_BIG_ENDIAN (RWAV: always big) */
    uint32_t version;                    /* packed NwVersion (RWAV: major << 24 | minor << 16) */
    int file_size;                       /* as stated in the header */
    int codec;                           /* VGA_NW_CODEC_* */
    int looping, loop_start;             /* a prefetch file reads as not looping (Common.cs:51) */
    int sample_count;                    /* RWAV: NibbleToSample of the stored address, whatever the codec;
                                          * prefetch: BytesToSamples(prefetch_size / channel_count, codec) */
    int sample_rate, channel_count;
    int channel_bytes;                   /* Common.SamplesToBytes(sample_count, codec): one channel's audio */
    int has_loop_start_unaligned;        /* CWAV / FWAV of a version with Common.IncludeUnalignedLoopWave */
    int loop_start_unaligned;
    /* prefetch files only (else 0): the first region of the PDAT block and the stream's interleave geometry.  Channel
     * c's byte p lies at prefetch_audio_offset + (p / il) * il * channel_count + c * cur + p % il, il = interleave_size
     * and cur = il, or for the last block what is left of prefetch_size / channel_count (Interleave.cs:118-167) */
    int prefetch_count, prefetch_start_sample, prefetch_size, prefetch_audio_offset;
    int stream_looping, stream_sample_count;   /* what the INFO block states for the whole stream */
    int interleave_count, interleave_size, samples_per_interleave, last_block_size_without_padding, last_block_samples,
        last_block_size;
    /* per channel; audio_offset counts from the start of the file (prefetch: the channel's first block) */
    int audio_offset[VGA_NW_MAX_CHANNELS];
    int16_t coefs[VGA_NW_MAX_CHANNELS][16];    /* GC-ADPCM only, zero for PCM */
    int16_t gain[VGA_NW_MAX_CHANNELS];         /* RWAV only */
    int16_t start_context[VGA_NW_MAX_CHANNELS][3];   /* predictor/scale, hist1, hist2 */
    int16_t loop_context[VGA_NW_MAX_CHANNELS][3];
} vga_nwwav_info;

/* host only; never reads outside [file, file + size).  VGA_ERR_INVALID_DATA with the reference's message for what its
 * readers reject (magic, byte order mark, block sizes that disagree, a file shorter than stated) and for what they
 * would read past the end of or index out of range: any offset or length outside the image, a prefetch count of 0, no
 * channels or more than 255, fewer GC-ADPCM channel infos or wave audio offsets than channels, an unknown codec, an
 * info and a data block of different kinds.  VGA_ERR_INVALID_OP for RSTM / CSTM / FSTM streams (vga_nwstm_parse). */
int vga_nwwav_parse(const uint8_t *file, size_t size, vga_nwwav_info *out);
/* host only: out[c] gets info->channel_bytes bytes as stored (PCM16 in the file's byte order) */
int vga_nwwav_read(const uint8_t *file, size_t size, const vga_nwwav_info *info, uint8_t *const *out);

/* ----------------------------------------------------------------------
 * A bank: nfiles parsed files of any mix of kinds, codecs, shapes and byte orders, file f's image file_offsets[f]
 * bytes into ONE device buffer.  Its channels are the bank's rows, in file order and channel order within a file;
 * each row goes to one of three packed outputs by its codec:
 *   d_adpcm  GC-ADPCM rows as stored.  Row i of the GC rows starts at exactly the byte offset that
 *            vga_gcadpcm_ragged_offsets gives for the sample counts of vga_nwwav_bank_gc_sample_counts, every row is
 *            zero-filled up to its 16 bytes and the 256 guard bytes after the last are zero: d_adpcm is a valid
 *            d_adpcm of vga_gcadpcm_decode_device_v for a vga_gcadpcm_ragged of those counts, with no further copy.
 *   d_pcm16  PCM16 rows as int16 in HOST order (ToShortArray(structure.Endianness)), rows rounded up to 8 samples.
 *   d_pcm8   PCM8 rows as stored (signed), rows rounded up to 16 bytes; vga_pcm8_decode_device with signed_ = 1 over
 *            the whole buffer as one row gives PCM16 at the same offsets.
 * Round-up bytes are written as zeros.  All three buffers must be 16-byte aligned (else VGA_ERR_ARGUMENT, nothing is
 * written) and hold what the size calls say (0: the pointer may be null); no byte outside them is written.  d_files
 * may lie at any byte.  create needs a device (the tables live in its memory); the object may be used by any
 * number of reads.
 * -------------------------------------------------------------------- */
typedef struct vga_nwwav_bank vga_nwwav_bank;
int vga_nwwav_bank_create(const vga_nwwav_info *infos, const int64_t *file_offsets, int nfiles, vga_nwwav_bank **out);
void vga_nwwav_bank_destroy(vga_nwwav_bank *bank);
int vga_nwwav_bank_channels(const vga_nwwav_bank *bank);                 /* all rows */
int vga_nwwav_bank_codec_channels(const vga_nwwav_bank *bank, int codec);   /* rows of one VGA_NW_CODEC_* */
/* per row (any pointer may be null): its file, its channel in the file, its codec, its sample count and where it
 * starts in its codec's output (bytes into d_adpcm / d_pcm8, samples into d_pcm16) */
int vga_nwwav_bank_rows(const vga_nwwav_bank *bank, int *file_out, int *channel_out, int *codec_out, int *sample_counts_out,
                        int64_t *offsets_out);
/* the GC-ADPCM rows in order: the sample counts vga_gcadpcm_ragged_create takes, and their coefficients (16 each),
 * start-context histories and gains ready for upload (any pointer may be null) */
int vga_nwwav_bank_gc_sample_counts(const vga_nwwav_bank *bank, int *sample_counts_out);
int vga_nwwav_bank_gc_tables(const vga_nwwav_bank *bank, int16_t *coefs_out, int16_t *hist1_out, int16_t *hist2_out,
                             int16_t *gain_out);
int64_t vga_nwwav_bank_adpcm_bytes(const vga_nwwav_bank *bank);   /* = vga_gcadpcm_ragged_adpcm_bytes; 0 without GC rows */
int64_t vga_nwwav_bank_pcm16_samples(const vga_nwwav_bank *bank);
int64_t vga_nwwav_bank_pcm8_bytes(const vga_nwwav_bank *bank);
int64_t vga_nwwav_bank_source_bytes(const vga_nwwav_bank *bank);  /* d_files must hold this much */
/* one launch on the caller's stream: no synchronisation, no allocation, no copy of tables */
int vga_nwwav_bank_read_device(const vga_nwwav_bank *bank, const uint8_t *d_files, uint8_t *d_adpcm, int16_t *d_pcm16,
                               uint8_t *d_pcm8, void *stream);

#ifdef __cplusplus
}
#endif
#endif

/*
 * oracle.h -- CPU restatement of the VGAudio codec hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under oracle/ is part of the product:
 * only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 * load this library, and only as the checker / reported CPU baseline.
 *
 * Every function cites the reference file:line it follows (paths relative to
 * /root/reference/src/VGAudio/).  The reference is C#; no .NET toolchain is
 * available in this image, so the reference itself cannot be built.  Parity
 * is pinned on the reference's own known-answer tests (see tests/), on
 * hand-derivable vectors, and on encoder/decoder self-consistency.
 *
 * Numeric model reproduced: RyuJIT x64 (SSE2 scalar f32/f64, no FMA
 * contraction, unchecked int32 wrap-around, arithmetic >>, truncating
 * integer division, Math.Round = ties-to-even).
 * Build flags: -O2 -ffp-contract=off -fexcess-precision=standard -fwrapv.
 */
#ifndef VGAUDIO_ORACLE_H
#define VGAUDIO_ORACLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- synthetic PCM16 of the benchmark (vgaudio_amd/synth.py in C; not part of the reference) ---- */
void vgo_synth_channel_params(int c, uint32_t out[4]);
void vgo_synth_channel(int c, int64_t first_sample, int n, int16_t *out);
void vgo_synth_generate(int16_t *out, long pitch, int nch, int n, int first_channel, int threads);

/* ---- GC-ADPCM size math: Codecs/GcAdpcm/GcAdpcmMath.cs:7-47 ---- */
int vgo_gc_nibble_count_to_sample_count(int nibble_count);
int vgo_gc_sample_count_to_nibble_count(int sample_count);
int vgo_gc_nibble_to_sample(int nibble);
int vgo_gc_sample_to_nibble(int sample);
int vgo_gc_sample_count_to_byte_count(int sample_count);
int vgo_gc_byte_count_to_sample_count(int byte_count);

/* ---- GC-ADPCM codec ---- */
/* Codecs/GcAdpcm/GcAdpcmCoefficients.cs:9-110 */
void vgo_gc_calculate_coefficients(const int16_t *pcm, int length, int16_t coefs[16]);
/* Codecs/GcAdpcm/GcAdpcmEncoder.cs:14-46.  sample_count == -1 -> pcm_length.
 * out must hold vgo_gc_sample_count_to_byte_count(sample_count) bytes.
 * Returns 0, or -1 if sample_count > pcm_length (the reference throws). */
int vgo_gc_encode(const int16_t *pcm, int pcm_length, const int16_t coefs[16],
                  int sample_count, int16_t hist1, int16_t hist2, uint8_t *out);
/* Codecs/GcAdpcm/GcAdpcmEncoder.cs:48-94 (one frame, in/out 16 shorts). */
void vgo_gc_encode_frame(int16_t pcm_inout[16], int sample_count, uint8_t adpcm_out[8],
                         const int16_t coefs[16]);
/* Codecs/GcAdpcm/GcAdpcmDecoder.cs:10-54 */
void vgo_gc_decode(const uint8_t *adpcm, const int16_t coefs[16], int sample_count,
                   int16_t hist1, int16_t hist2, int16_t *pcm_out);

/* Formats/GcAdpcm/GcAdpcmFormat.cs:58-74,129-135 -- batch driver with the
 * reference's scheduling (one task per channel on `threads` workers; the
 * reference uses Parallel.For).  pcm: planar, channel c at pcm + c*pitch.
 * adpcm_out: channel c at adpcm_out + c*out_pitch.  coefs_out: nch*16. */
void vgo_gc_encode_batch(const int16_t *pcm, long pitch, int nch, int sample_count,
                         int16_t *coefs_out, uint8_t *adpcm_out, long out_pitch,
                         int threads);
void vgo_gc_decode_batch(const uint8_t *adpcm, long in_pitch, const int16_t *coefs, int nch,
                         int sample_count, int16_t *pcm_out, long out_pitch, int threads);

/* ---- GC-ADPCM channel metadata: what GcAdpcmChannelBuilder derives when a channel is built
 * (Formats/GcAdpcm/GcAdpcmChannelBuilder.cs:148-202), SURVEY.md 8f rank 1 ---- */
typedef struct {
    int sample_count;                   /* GcAdpcmChannelBuilder.SampleCount (unaligned) */
    int looping, loop_start, loop_end;  /* WithLoop; not looping -> 0, 0 (:103-120) */
    int loop_alignment_multiple;        /* WithLoopAlignment (:64-68); 0 = none */
    int samples_per_seek_table_entry;   /* WithSamplesPerSeekTableEntry (:78-87); 0 = no seek table */
} vgo_gc_channel_params;
typedef struct {
    int alignment_needed;               /* GcAdpcmAlignment.AlignmentNeeded (GcAdpcmAlignment.cs:25) */
    int loop_start_aligned;             /* LoopStartAligned, or loop_start when no alignment is needed */
    int sample_count_aligned;           /* SampleCountAligned, or sample_count */
    int seek_table_entries;             /* DivideByRoundUp(pcm length, samples per entry), or 0 */
} vgo_gc_channel_layout;
/* size math only; returns 0 */
int vgo_gc_channel_layout_for(const vgo_gc_channel_params *p, vgo_gc_channel_layout *out);
/* GcAdpcmAlignment ctor (GcAdpcmAlignment.cs:20-63).  adpcm_aligned_out: SampleCountToByteCount(
 * sample_count_aligned) bytes, pcm_aligned_out: sample_count_aligned shorts (only written when
 * alignment is needed).  Returns 0; -4 when loop_start == loop_end needs alignment (the reference's
 * fill loop `currentSample += loopLength` never ends). */
int vgo_gc_alignment(int multiple, int loop_start, int loop_end, const uint8_t *adpcm, const int16_t coefs[16],
                     vgo_gc_channel_layout *layout, uint8_t *adpcm_aligned_out, int16_t *pcm_aligned_out);
/* GcAdpcmLoopContext(byte[] adpcm, short[] pcm, int loopStart) (GcAdpcmLoopContext.cs:17-26): out = pred/scale
 * byte, hist1, hist2.  pcm may be NULL (hist 0). */
void vgo_gc_loop_context(const uint8_t *adpcm, const int16_t *pcm, int loop_start, int16_t out[3]);
/* GcAdpcmChannel(GcAdpcmChannelBuilder) for a freshly encoded channel (GcAdpcmChannel.cs:31-55 ->
 * GetAlignment / GetLoopContext / GetSeekTable, no previous caches).  Outputs sized by
 * vgo_gc_channel_layout_for; any of them may be NULL.  adpcm_out / pcm_out receive GetAdpcmAudio() /
 * the decoded PCM the builder ends up holding (aligned or not).  Returns 0, -4 (see vgo_gc_alignment)
 * or -2 when the loop context's pred/scale byte lies past the ORIGINAL adpcm array (the reference
 * reads b.Adpcm, not the aligned copy, :179 -- IndexOutOfRangeException). */
int vgo_gc_build_channel(const uint8_t *adpcm, const int16_t coefs[16], const vgo_gc_channel_params *p,
                         vgo_gc_channel_layout *layout_out, uint8_t *adpcm_out, int16_t *pcm_out,
                         int16_t *seek_table_out, int16_t loop_context_out[3]);

/* ---- DSP container (Containers/Dsp/DspWriter.cs, DspReader.cs), SURVEY.md 8f rank 2 ---- */
typedef struct {
    int sample_rate;
    int sample_count;                 /* GcAdpcmFormat.SampleCount */
    int looping, loop_start, loop_end;/* GcAdpcmFormat.Looping / LoopStart / LoopEnd */
    int samples_per_interleave;       /* DspConfiguration.SamplesPerInterleave, default 0x3800 */
    int loop_point_alignment;         /* DspConfiguration.LoopPointAlignment, default 1 */
    int trim_file;                    /* Configuration.TrimFile, default true */
} vgo_dsp_params;
typedef struct {
    int sample_count, loop_start, loop_end;            /* as written to the header (DspWriter.cs:22,29-31) */
    int start_addr, end_addr, cur_addr;                /* :33-35 */
    int bytes_per_interleave, frames_per_interleave;   /* :25-27 */
    int audio_data_size, file_size;                    /* :99-100, :18 */
} vgo_dsp_layout;
typedef struct {
    int sample_count, nibble_count, sample_rate, looping, format, start_addr, end_addr, cur_addr;
    int channel_count, frames_per_interleave;
} vgo_dsp_header;
void vgo_interleave(const uint8_t *const *inputs, int count, int input_size, int interleave, int output_size, uint8_t *out);
int vgo_deinterleave(const uint8_t *in, int in_len, int interleave, int count, int output_size, uint8_t *const *outs);
int vgo_dsp_layout_for(const vgo_dsp_params *p, int nch, vgo_dsp_layout *out);
int vgo_dsp_write(const uint8_t *const *adpcm, int adpcm_len, const int16_t *coefs, const int16_t *gain,
                  const int16_t *start_context, const int16_t *loop_context, int nch, const vgo_dsp_params *p,
                  uint8_t *file_out);
int vgo_dsp_read(const uint8_t *file, int file_len, vgo_dsp_header *hdr, int16_t *coefs_out, int16_t *gain_out,
                 int16_t *start_context_out, int16_t *loop_context_out, uint8_t *const *adpcm_out);

/* Formats/GcAdpcm/GcAdpcmSeekTable.cs:25-38 (CreateSeekTable).
 * table_out holds 2*ceil(n/samples_per_entry) shorts. */
void vgo_gc_create_seek_table(const int16_t *pcm, int n, int samples_per_entry, int16_t *table_out);

/* statistics of the last vgo_gc_encode call on this thread: number of
 * quantise passes executed by DspEncodeCoef (GcAdpcmEncoder.cs:127-170)
 * histogrammed by trip count 1..15 (index 0 unused). */
void vgo_gc_trip_histogram(uint64_t hist_out[16]);
/* 1 if the last vgo_gc_encode on this thread reached the state in which the reference's
 * retry loop (GcAdpcmEncoder.cs:127-170) never terminates (see gcadpcm_oracle.c). */
int vgo_gc_last_encode_hit_nontermination(void);

/* ---- CRI ADX ---- Codecs/CriAdx/CriAdxCodec.cs */
typedef struct {
    int sample_rate;         /* 48000 */
    int highpass_frequency;  /* 500 */
    int frame_size;          /* 18 */
    int version;             /* 4 */
    int16_t history;         /* in/out for encode (CriAdxCodec.cs:73) */
    int padding;
    int type;                /* 2 Fixed, 3 Linear, 4 Exponential */
    int filter;
} vgo_adx_params;

void vgo_adx_default_params(vgo_adx_params *p);
/* CriAdxCodec.cs:173-184 */
void vgo_adx_calculate_coefficients(int highpass_freq, int sample_rate, int16_t coefs[2]);
/* number of bytes Encode allocates: frameCount * FrameSize (CriAdxCodec.cs:59-66) */
int vgo_adx_encoded_size(int pcm_length, const vgo_adx_params *p);
/* CriAdxCodec.cs:56-105; updates p->history like the reference */
void vgo_adx_encode(const int16_t *pcm, int pcm_length, vgo_adx_params *p, uint8_t *out);
/* CriAdxCodec.cs:9-54 */
void vgo_adx_decode(const uint8_t *adpcm, int sample_count, const vgo_adx_params *p, int16_t *pcm_out);
/* Formats/CriAdx/CriAdxHelpers.cs:7-31 */
int vgo_adx_nibble_count_to_sample_count(int nibble_count, int frame_size);
int vgo_adx_sample_count_to_nibble_count(int sample_count, int frame_size);
int vgo_adx_sample_count_to_byte_count(int sample_count, int frame_size);
void vgo_adx_encode_batch(const int16_t *pcm, long pitch, int nch, int pcm_length,
                          const vgo_adx_params *p, uint8_t *out, long out_pitch,
                          int16_t *history_out, int threads);
void vgo_adx_decode_batch(const uint8_t *adpcm, long in_pitch, int nch, int sample_count,
                          const vgo_adx_params *p, int16_t *pcm_out, long out_pitch, int threads);


/* ---- CRI HCA ---- Codecs/CriHca (all files), Utilities/{Mdct,BitWriter,BitReader,Crc16}.cs */
typedef struct {            /* Codecs/CriHca/HcaInfo.cs:5-50 (fields the codec path uses) */
    int channel_count, sample_rate, sample_count, frame_count;
    int inserted_samples, appended_samples, header_size, frame_size;
    int min_resolution, max_resolution, track_count, channel_config;
    int total_band_count, base_band_count, stereo_band_count, hfr_band_count;
    int bands_per_hfr_group, hfr_group_count;
    int looping, loop_start_frame, loop_end_frame, pre_loop_samples, post_loop_samples;
    int use_ath_curve, comment_length;
} vgo_hca_info;

typedef struct {            /* Codecs/CriHca/CriHcaParameters.cs:3-15; quality: 1 Highest .. 5 Lowest, 0 NotSet */
    int quality, bitrate, limit_bitrate, channel_count, sample_rate, sample_count;
    int looping, loop_start, loop_end;
} vgo_hca_params;

/* CriHcaEncoder.Initialize (CriHcaEncoder.cs:61-114): 0, or -2 (ArgumentOutOfRange) */
int vgo_hca_encoder_init(const vgo_hca_params *c, vgo_hca_info *h, int *post_samples_out, int *buffer_pre_samples_out);
/* CriHcaFormat.EncodeFromPcm16 (Formats/CriHca/CriHcaFormat.cs:34-84): pcm planar (channel c at
 * pcm + c*pitch); frames_out = frame_count*frame_size bytes.  0, -2, -3 (InvalidData: bitrate too low) */
int vgo_hca_encode(const int16_t *pcm, long pitch, const vgo_hca_params *c, vgo_hca_info *info_out, uint8_t *frames_out);
/* CriHcaDecoder.Decode (CriHcaDecoder.cs:11-45): pcm_out planar, sample_count samples per channel.  0; -2 (no or more than
 * 8 channels, track count below 1); -3 (InvalidData: a bad sync word); -6 (IndexOutOfRangeException: intensity 15, more
 * than 128 coded bands or 8 HFR groups, HFR or stereo bands past 128, too few channels per track for the channel
 * types) -- at the frame where the reference throws; the PCM of the frames before it is kept */
int vgo_hca_decode(const vgo_hca_info *h, const uint8_t *frames, int16_t *pcm_out, long pitch);
int vgo_hca_encode_batch(const int16_t *pcm, long stream_pitch, long ch_pitch, int nstreams, const vgo_hca_params *p,
                         uint8_t *frames, long frames_pitch, int threads);
int vgo_hca_decode_batch(const vgo_hca_info *info, const uint8_t *frames, long frames_pitch, int nstreams,
                         int16_t *pcm_out, long stream_pitch, long ch_pitch, int threads);
/* Which way the data-dependent decisions of CriHcaEncoder.EncodeFrame went during this thread's last vgo_hca_encode
 * (zeroed at its start; counting changes no output byte).  Frames that end in an error are counted up to the error. */
typedef struct {
    uint64_t frames;                    /* EncodeFrame calls */
    uint64_t sf_delta_bits[7];          /* channel headers written, by CriHcaChannel.ScaleFactorDeltaBits (6: raw) */
    uint64_t intensity[14];             /* primary sub-frames by the intensity index stored (:741-755; 13: the bound) */
    uint64_t hfr_zero, hfr_sqrt2, hfr_inverse;   /* HFR groups: average 0, scale sqrt(2), scale 1 / average (:824-827) */
    uint64_t band_drops;                /* iterations of CalculateNoiseLevel's retry loop (:466-482) */
    uint64_t band_drops_frame_max;      /* the most of them in one frame */
    uint64_t frames_with_band_drops, frames_with_repeated_band_drops;
    uint64_t frames_level_zero;         /* CalculateEvaluationBoundary returns early (:489-493) */
    uint64_t boundary_exit_equal;       /* BinarySearchBoundary ends at low == high (:544-547) */
    uint64_t boundary_exit_probe;       /* ... or at the final probe of `high` (:549-551) */
    uint64_t frames_level_search_hit_255;   /* a BinarySearchLevel of the frame ended at low == 255 */
    uint64_t error_minus3, error_minus4;    /* frames that ended in "Bitrate is set too low" / NotImplementedException */
} vgo_hca_encode_paths;
void vgo_hca_encode_paths_get(vgo_hca_encode_paths *out);
/* test hooks */
int vgo_hca_table(const char *name, double *out, int cap);
uint16_t vgo_crc16(const uint8_t *data, int size);                       /* Utilities/Crc16.cs:12-18 */

/* ---- ADX / HCA containers (adxhca_container_oracle.c): Containers/Adx/AdxWriter.cs, Containers/Hca/HcaWriter.cs ---- */
typedef struct {
    int sample_rate;
    int sample_count;                  /* CriAdxFormat.SampleCount (= unaligned + AlignmentSamples) */
    int looping, loop_start, loop_end; /* CriAdxFormat.Looping / LoopStart / LoopEnd (aligned) */
    int alignment_samples;             /* CriAdxFormat.AlignmentSamples */
    int frame_size, version, type;     /* type: 2 Fixed, 3 Linear, 4 Exponential */
    int highpass_frequency;
    int encryption_type;               /* AdxConfiguration.EncryptionType (header byte only) */
    int trim_file;
} vgo_adxfile_params;
typedef struct {
    int sample_count, frame_count, base_header_size, alignment_bytes, header_size, audio_offset, audio_size;
    int footer_offset, footer_size, loop_start_offset, loop_end_offset, file_size;
} vgo_adxfile_layout;
typedef struct {
    int header_size, type, frame_size, bit_depth, channel_count, sample_rate, sample_count, highpass_frequency;
    int version, revision, inserted_samples, loop_count, looping, loop_type;
    int loop_start_sample, loop_start_byte, loop_end_sample, loop_end_byte;
} vgo_adxfile_header;
int vgo_adxfile_layout_for(const vgo_adxfile_params *p, int nch, vgo_adxfile_layout *out);
int vgo_adxfile_write(const uint8_t *const *audio, int audio_len, const int16_t *history, int nch,
                      const vgo_adxfile_params *p, uint8_t *file_out);
int vgo_adxfile_read(const uint8_t *file, int file_len, vgo_adxfile_header *h, int16_t *history_out, uint8_t *const *audio_out);
int vgo_hcafile_size(const vgo_hca_info *h);
int vgo_hcafile_write(const vgo_hca_info *h, const uint8_t *frames, const char *comment, float volume, int encryption_type,
                      int encrypted_ids, uint8_t *file_out);
int vgo_hcafile_read(const uint8_t *file, int file_len, vgo_hca_info *h, float *volume_out, int *encryption_type_out,
                     char *comment_out, int *version_out);

/* ---- WAVE 16-bit PCM (wave_oracle.c): Containers/Wave/WaveReader.cs, WaveWriter.cs, Utilities/Riff ---- */
typedef struct {
    int channel_count, sample_rate, bits_per_sample;
    int sample_count;            /* per channel, from the data bytes actually present (what the Pcm16Format holds) */
    int sample_count_declared;   /* from the data chunk's declared size (WaveStructure.SampleCount) */
    int looping, loop_start, loop_end;
    int smpl_loop_count, smpl_loop_start, smpl_loop_end;
    long data_offset;
    int data_size, data_size_declared;
} vgo_wave_info;
typedef struct { int sample_rate, sample_count, looping, loop_start, loop_end; } vgo_wave_params;
int vgo_wave_parse(const uint8_t *file, long file_len, vgo_wave_info *out);
int vgo_wave_read_pcm16(const uint8_t *file, long file_len, const vgo_wave_info *w, int16_t *const *pcm_out);
long vgo_wave_file_size(const vgo_wave_params *p, int nch);
int vgo_wave_write_pcm16(const int16_t *const *pcm, int nch, const vgo_wave_params *p, uint8_t *file_out);

/* ---- ADX / HCA encryption (crypt_oracle.c): Codecs/CriAdx/CriAdxKey.cs, CriAdxEncryption.cs, Codecs/CriHca/CriHcaKey.cs,
 * CriHcaEncryption.cs ---- */
typedef struct { int seed, mult, inc; } vgo_adx_key;
void vgo_adx_key_from_code(uint64_t key_code, vgo_adx_key *k);
void vgo_adx_key_from_string(const char *s, vgo_adx_key *k);
uint64_t vgo_adx_key_code(const vgo_adx_key *k);
void vgo_adx_crypt_channel(uint8_t *adpcm, int adpcm_len, const vgo_adx_key *key, int encryption_type, int frame_size,
                           int channel_num, int channel_count);
int vgo_adx_test_key(const uint8_t *const *adpcm, int adpcm_len, int nch, const vgo_adx_key *key, int encryption_type, int frame_size);
int vgo_hca_key_tables(int key_type, uint64_t key_code, uint8_t decryption[256], uint8_t encryption[256]);
void vgo_hca_crypt(uint8_t *frames, int frame_count, int frame_size, const uint8_t table[256]);
/* CriHcaEncryption.FindKey over caller-supplied decryption tables (hca_oracle.c); -1 none, -3 bad sync word */
int vgo_hca_find_key(const vgo_hca_info *h, const uint8_t *frames, int frame_count, const uint8_t *tables, int nkeys);
/* VGAudio.Tools/CrackAdx/GuessAdx.cs: the brute-force key search for one file's frame scales */
int vgo_adx_default_candidates(int encryption_type, int *mults, int *nmult, int *incs, int *ninc);
int vgo_adx_guess_keys(const uint16_t *scales, int nscales, int start_frame, int encryption_type, const int *mults,
                       int nmult, const int *incs, int ninc, vgo_adx_key *out, int max_keys);
/* VGAudio.Tools/CrackHca/Crack.cs:43-80: byte-value counts at the first `positions` bytes of every frame */
void vgo_hca_byte_position_counts(const uint8_t *frames, long frames_pitch, int nstreams, int frame_count, int frame_size,
                                  int positions, uint32_t *counts);
int vgo_bitwriter_write(uint8_t *buf, int buf_len, int position, int value, int bit_count);  /* BitWriter.cs:26-70 */
void vgo_mdct_run(const double *in, int blocks, double *out, int inverse);   /* Mdct.cs:63-119, 128-point, HCA scale */
int vgo_hca_debug_last_frame(const int16_t *pcm, long pitch, const vgo_hca_params *c, int frames,
                             int *noise_level, int *eval_boundary, int *scale_factors, int *resolution,
                             int *quantized, double *spectra);

#ifdef __cplusplus
}
#endif
#endif

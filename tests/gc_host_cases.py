"""The case tables of tests/test_gc_host_layer.py (test code only), and the generator of the refusals recorded in
tests/golden/gc_host_refusals.json:

    python tests/gc_host_cases.py [--library PATH/libvgaudio_hip.so]

runs every refused call below on a build of the PARENT of the change that moved the GC-ADPCM host layer into
csrc/gc_host.hpp and writes each call's code and message: the yardstick is that library, not the moved code.  Every call
is one an argument test refuses before anything reaches the device, so the table needs no GPU; data pointers are never
dereferenced on those paths and are dummy addresses, the row and count arrays are real."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(HERE, "golden", "gc_host_refusals.json")

# ---- layout cases: vga_gcadpcm_channel_params = (sample_count, looping, loop_start, loop_end, loop_alignment_multiple,
# samples_per_seek_table_entry) with a channel count for the workspace; `null`: 1 = no parameters, 2 = no output
CHANNEL_CASES = {
    "no_loop": ((100000, 0, 0, 0, 0, 0), 2, 0),
    "no_loop_seek_0x3800": ((100000, 0, 0, 0, 0, 0x3800), 2, 0),
    "empty": ((0, 0, 0, 0, 0, 0x3800), 1, 0),
    "aligned_loop": ((100000, 1, 14336, 90000, 14336, 0x3800), 2, 0),
    "aligned_loop_multiple_1": ((100000, 1, 1234, 90000, 1, 0x3800), 3, 0),
    "multiple_0": ((100000, 1, 1234, 90000, 0, 0x3800), 2, 0),
    "unaligned_loop": ((100000, 1, 1234, 90000, 14336, 0x3800), 2, 0),
    "unaligned_loop_seek_0": ((100000, 1, 15000, 99999, 14336, 0), 16, 0),
    "unaligned_loop_seek_1": ((5000, 1, 3, 4000, 14, 1), 1, 0),
    "zero_length_loop_unaligned": ((5000, 1, 100, 100, 14336, 0x3800), 2, 0),
    "loop_past_the_data": ((1000, 1, 900, 20000, 14336, 0x3800), 2, 0),
    "no_channels": ((100000, 1, 1234, 90000, 14336, 0x3800), 0, 0),
    "refused_null_params": ((0, 0, 0, 0, 0, 0), 2, 1),
    "refused_null_output": ((100000, 0, 0, 0, 0, 0), 2, 2),
    "refused_out_of_range": ((100000, 1, 90000, 1234, 14336, 0x3800), 2, 0),
    "refused_overflow": ((2**31 - 1, 1, 1, 2**31 - 20, 14336, 0x3800), 2, 0),
}
# vga_dsp_params = (sample_rate, sample_count, looping, loop_start, loop_end, samples_per_interleave,
# loop_point_alignment, trim_file) with a channel count
DSP_CASES = {
    "mono_no_loop": ((48000, 100000, 0, 0, 0, 14336, 0, 0), 1, 0),
    "stereo_no_loop": ((48000, 100001, 0, 0, 0, 14336, 0, 0), 2, 0),
    "aligned_loop": ((32000, 100000, 1, 14336, 90000, 14336, 14336, 0), 2, 0),
    "unaligned_loop": ((32000, 100000, 1, 1234, 90000, 14336, 14336, 0), 2, 0),
    "unaligned_loop_trimmed": ((32000, 100000, 1, 1234, 90000, 14, 14336, 1), 6, 0),
    "alignment_1": ((32000, 100000, 1, 1234, 90000, 14336, 1, 1), 2, 0),
    "loop_beyond_the_samples": ((32000, 1000, 1, 10, 5000, 14336, 0, 0), 2, 0),
    "empty": ((32000, 0, 0, 0, 0, 14, 0, 0), 1, 0),
    "refused_null_params": ((0,) * 8, 2, 1),
    "refused_null_output": ((48000, 100000, 0, 0, 0, 14336, 0, 0), 2, 2),
    "refused_no_channels": ((48000, 100000, 0, 0, 0, 14336, 0, 0), 0, 0),
    "refused_interleave_0": ((48000, 100000, 0, 0, 0, 0, 0, 0), 2, 0),
    "refused_interleave_15": ((48000, 100000, 0, 0, 0, 15, 0, 0), 2, 0),
    "refused_negative": ((48000, -1, 0, 0, 0, 14336, 0, 0), 2, 0),
    "refused_2_gib": ((48000, 1_800_000_000, 0, 0, 0, 14336, 0, 0), 3, 0),
    "nibbles_wrap": ((48000, 2**31 - 100, 0, 0, 0, 14336, 0, 0), 2, 0),          # int arithmetic wraps, as the reference's
}

# ---- refused calls into the product library.  Arguments: an int is itself (a dummy address where the parameter is a
# pointer), None a null pointer, ("rows", ...) an array of pointers, ("ints", ...) an int array, ("chan", ...) and ("dsp",
# ...) the parameter structs above.
A, B = 0x100000, 0x200000              # aligned dummy addresses
ROWS2, NULLROW = ("rows", A, B), ("rows", A, None)
CHAN_OK = ("chan", 100000, 0, 0, 0, 0, 0x3800)
CHAN_BAD = ("chan", 100000, 1, 90000, 1234, 14336, 0x3800)
CHAN_UNALIGNED = ("chan", 100000, 1, 1234, 90000, 14336, 0x3800)
CHAN_ZERO_LOOP = ("chan", 5000, 1, 100, 100, 14336, 0)
CHAN_LOOP_PAST = ("chan", 1000, 1, 900, 20000, 14336, 0)
DSP_OK = ("dsp", 48000, 100000, 0, 0, 0, 14336, 0, 0)
DSP_BAD = ("dsp", 48000, 100000, 0, 0, 0, 15, 0, 0)
BIG = 1 << 40                          # a workspace size that is always enough

REFUSED_CALLS = {
    # the device entry points
    "coefs_device/negative": ("vga_gcadpcm_coefs_device", [A, 1000, -1, 1000, A, A, BIG, None]),
    "coefs_device/negative_length_and_misaligned": ("vga_gcadpcm_coefs_device", [A + 2, 1000, 2, -1, A, A, BIG, None]),
    "coefs_device/misaligned": ("vga_gcadpcm_coefs_device", [A + 2, 1000, 2, 1000, A, A, BIG, None]),
    "coefs_device/odd_pitch": ("vga_gcadpcm_coefs_device", [A, 1001, 2, 1000, A, A, BIG, None]),
    "coefs_device/short_pitch_and_no_workspace": ("vga_gcadpcm_coefs_device", [A, 998, 2, 1000, A, None, 0, None]),
    "coefs_device/small_workspace": ("vga_gcadpcm_coefs_device", [A, 1000, 2, 1000, A, A, 16, None]),
    "coefs_device/null_workspace": ("vga_gcadpcm_coefs_device", [A, 1000, 2, 1000, A, None, BIG, None]),
    "encode_device/negative": ("vga_gcadpcm_encode_device", [A, 1000, 2, -1, A, None, None, A, 576, None]),
    "encode_device/misaligned_base_and_short_pitch": ("vga_gcadpcm_encode_device", [A + 2, 998, 2, 1000, A, None, None, A, 576, None]),
    "encode_device/bad_pcm_and_bad_adpcm": ("vga_gcadpcm_encode_device", [A, 999, 2, 1000, A, None, None, A + 4, 100, None]),
    "encode_device/adpcm_misaligned": ("vga_gcadpcm_encode_device", [A, 1000, 2, 1000, A, None, None, A + 4, 576, None]),
    "encode_device/adpcm_pitch_short": ("vga_gcadpcm_encode_device", [A, 1000, 2, 1000, A, None, None, A, 568, None]),
    "encode_device/adpcm_pitch_not_8": ("vga_gcadpcm_encode_device", [A, 1000, 2, 1000, A, None, None, A, 580, None]),
    "decode_device/negative": ("vga_gcadpcm_decode_device", [A, 576, A, -2, 1000, None, None, A, 1000, None, None]),
    "decode_device/bad_pcm_and_bad_adpcm": ("vga_gcadpcm_decode_device", [A + 1, 8, A, 2, 1000, None, None, A + 2, 10, None, None]),
    "decode_device/adpcm_misaligned": ("vga_gcadpcm_decode_device", [A + 4, 576, A, 2, 1000, None, None, A, 1000, None, None]),
    "synth/short_pitch": ("vga_synth_pcm16_device", [A, 10, 2, 100, 0, A, None]),
    "synth/negative": ("vga_synth_pcm16_device", [A, 100, -1, 100, 0, A, None]),
    # channel metadata on the device
    "build_device/null_params_and_negative": ("vga_gcadpcm_build_channels_device", [A, 57144, A, -1, None, A, 57144, None, 0, None, 0, None, A, BIG, None]),
    "build_device/bad_params_and_negative": ("vga_gcadpcm_build_channels_device", [A, 57144, A, -1, CHAN_BAD, A, 57144, None, 0, None, 0, None, A, BIG, None]),
    "build_device/negative_and_misaligned": ("vga_gcadpcm_build_channels_device", [A + 4, 57144, A, -1, CHAN_OK, A, 57144, None, 0, None, 0, None, A, BIG, None]),
    "build_device/input_misaligned_and_output_missing": ("vga_gcadpcm_build_channels_device", [A + 4, 57144, A, 2, CHAN_UNALIGNED, None, 0, None, 0, None, 0, None, A, BIG, None]),
    "build_device/output_missing_and_bad_pcm": ("vga_gcadpcm_build_channels_device", [A, 57144, A, 2, CHAN_UNALIGNED, None, 0, A + 2, 10, None, 0, None, A, BIG, None]),
    "build_device/bad_output_and_bad_pcm": ("vga_gcadpcm_build_channels_device", [A, 57144, A, 2, CHAN_OK, A + 4, 57144, A + 2, 10, None, 0, None, A, BIG, None]),
    "build_device/bad_pcm_and_short_seek_pitch": ("vga_gcadpcm_build_channels_device", [A, 57144, A, 2, CHAN_OK, A, 57144, A + 2, 10, A, 2, None, A, BIG, None]),
    "build_device/short_seek_pitch_and_small_workspace": ("vga_gcadpcm_build_channels_device", [A, 57144, A, 2, CHAN_OK, A, 57144, A, 100000, A, 2, None, A, 16, None]),
    "build_device/small_workspace": ("vga_gcadpcm_build_channels_device", [A, 57144, A, 2, CHAN_OK, A, 57144, A, 100000, A, 16, None, A, 16, None]),
    "build_device/null_workspace": ("vga_gcadpcm_build_channels_device", [A, 57144, A, 2, CHAN_OK, A, 57144, A, 100000, A, 16, None, None, BIG, None]),
    "build_device/workspace_misaligned": ("vga_gcadpcm_build_channels_device", [A, 57144, A, 2, CHAN_OK, A, 57144, A, 100000, A, 16, None, A + 8, BIG, None]),
    "build_device/small_workspace_and_loop_past_the_data": ("vga_gcadpcm_build_channels_device", [A, 57144, A, 2, CHAN_LOOP_PAST, A, 57144, None, 0, None, 0, A, A, 16, None]),
    "build_device/loop_context_past_the_data": ("vga_gcadpcm_build_channels_device", [A, 57144, A, 2, CHAN_LOOP_PAST, A, 57144, None, 0, None, 0, A, A, BIG, None]),
    "build_device/zero_length_loop": ("vga_gcadpcm_build_channels_device", [A, 57144, A, 2, CHAN_ZERO_LOOP, A, 57144, None, 0, None, 0, None, A, BIG, None]),
    "build_device/zero_length_loop_with_context": ("vga_gcadpcm_build_channels_device", [A, 57144, A, 2, CHAN_ZERO_LOOP, A, 57144, None, 0, None, 0, A, A, BIG, None]),
    # ... and from host rows
    "build_batch/bad_params_and_null_rows": ("vga_gcadpcm_build_channels_batch", [None, A, 2, CHAN_BAD, None, None, None, None]),
    "build_batch/negative_and_null_rows": ("vga_gcadpcm_build_channels_batch", [None, None, -1, CHAN_OK, None, None, None, None]),
    "build_batch/null_rows_and_null_coefs": ("vga_gcadpcm_build_channels_batch", [None, None, 2, CHAN_OK, None, None, None, None]),
    "build_batch/null_row": ("vga_gcadpcm_build_channels_batch", [NULLROW, A, 2, CHAN_OK, None, None, None, None]),
    "build_batch/null_coefs_and_output_missing": ("vga_gcadpcm_build_channels_batch", [ROWS2, None, 2, CHAN_UNALIGNED, None, None, None, None]),
    "build_batch/output_missing": ("vga_gcadpcm_build_channels_batch", [ROWS2, A, 2, CHAN_UNALIGNED, None, NULLROW, None, None]),
    "build_batch/null_output_row_and_null_pcm_row": ("vga_gcadpcm_build_channels_batch", [ROWS2, A, 2, CHAN_OK, NULLROW, NULLROW, None, None]),
    "build_batch/null_pcm_row_and_null_seek_row": ("vga_gcadpcm_build_channels_batch", [ROWS2, A, 2, CHAN_OK, ROWS2, NULLROW, NULLROW, None]),
    "build_batch/null_seek_row": ("vga_gcadpcm_build_channels_batch", [ROWS2, A, 2, CHAN_OK, ROWS2, ROWS2, NULLROW, None]),
    # the DSP container
    "dsp_device/bad_params_and_negative": ("vga_dsp_write_device", [A, 57144, -1, None, None, None, None, 2, DSP_BAD, None, None]),
    "dsp_device/no_channels": ("vga_dsp_write_device", [A, 57144, 57144, A, None, None, None, 0, DSP_OK, A, None]),
    "dsp_device/negative_and_misaligned": ("vga_dsp_write_device", [A + 4, 57144, -1, A, None, None, None, 2, DSP_OK, A, None]),
    "dsp_device/null_coefs": ("vga_dsp_write_device", [A, 57144, 57144, None, None, None, None, 2, DSP_OK, A, None]),
    "dsp_device/null_file_and_misaligned": ("vga_dsp_write_device", [A + 4, 57144, 57144, A, None, None, None, 2, DSP_OK, None, None]),
    "dsp_device/null_audio": ("vga_dsp_write_device", [None, 57144, 57144, A, None, None, None, 2, DSP_OK, A, None]),
    "dsp_device/misaligned_audio_and_file": ("vga_dsp_write_device", [A + 4, 57144, 57144, A, None, None, None, 2, DSP_OK, A + 4, None]),
    "dsp_device/short_pitch": ("vga_dsp_write_device", [A, 57136, 57144, A, None, None, None, 2, DSP_OK, A, None]),
    "dsp_device/misaligned_file_and_short_mono": ("vga_dsp_write_device", [A, 64, 64, A, None, None, None, 1, DSP_OK, A + 4, None]),
    "dsp_device/short_mono": ("vga_dsp_write_device", [A, 64, 64, A, None, None, None, 1, DSP_OK, A, None]),
    "dsp_write/bad_params_and_negative": ("vga_dsp_write", [None, -1, None, None, None, None, 2, DSP_BAD, None]),
    "dsp_write/negative_and_null_rows": ("vga_dsp_write", [None, -1, A, None, None, None, 2, DSP_OK, A]),
    "dsp_write/null_rows_and_null_coefs": ("vga_dsp_write", [None, 100, None, None, None, None, 2, DSP_OK, A]),
    "dsp_write/null_row": ("vga_dsp_write", [NULLROW, 100, A, None, None, None, 2, DSP_OK, A]),
    "dsp_write/null_coefs": ("vga_dsp_write", [ROWS2, 100, None, None, None, None, 2, DSP_OK, A]),
    "dsp_write/null_output": ("vga_dsp_write", [ROWS2, 100, A, None, None, None, 2, DSP_OK, None]),
    # the equal-length host batches
    "coefs_batch/negative_length_and_null_rows": ("vga_gcadpcm_calculate_coefficients_batch", [None, 2, -1, A]),
    "coefs_batch/negative_count_and_null_rows": ("vga_gcadpcm_calculate_coefficients_batch", [None, -1, 100, None]),
    "coefs_batch/null_rows_and_null_coefs": ("vga_gcadpcm_calculate_coefficients_batch", [None, 2, 100, None]),
    "coefs_batch/null_row": ("vga_gcadpcm_calculate_coefficients_batch", [NULLROW, 2, 100, A]),
    "coefs_batch/null_coefs": ("vga_gcadpcm_calculate_coefficients_batch", [ROWS2, 2, 100, None]),
    "coefs_batch/null_coefs_empty": ("vga_gcadpcm_calculate_coefficients_batch", [None, 2, 0, None]),
    "coefs_batch/negative_count_empty": ("vga_gcadpcm_calculate_coefficients_batch", [None, -1, 0, A]),
    "encode_with_coefs/negative_and_null_rows": ("vga_gcadpcm_encode_with_coefs_batch", [None, 2, -2, -2, None, None, None, None]),
    "encode_with_coefs/count_above_length": ("vga_gcadpcm_encode_with_coefs_batch", [None, 2, 100, 101, None, None, None, None]),
    "encode_with_coefs/negative_count_and_null_row": ("vga_gcadpcm_encode_with_coefs_batch", [NULLROW, -1, 100, 100, None, None, None, None]),
    "encode_with_coefs/null_rows": ("vga_gcadpcm_encode_with_coefs_batch", [None, 2, 100, -1, None, None, None, None]),
    "encode_with_coefs/null_row_and_null_out": ("vga_gcadpcm_encode_with_coefs_batch", [NULLROW, 2, 100, 100, A, None, None, None]),
    "encode_with_coefs/null_out_and_null_coefs": ("vga_gcadpcm_encode_with_coefs_batch", [ROWS2, 2, 100, 100, None, None, None, None]),
    "encode_with_coefs/null_out_row": ("vga_gcadpcm_encode_with_coefs_batch", [ROWS2, 2, 100, 100, A, None, None, NULLROW]),
    "encode_with_coefs/null_coefs": ("vga_gcadpcm_encode_with_coefs_batch", [ROWS2, 2, 100, 100, None, None, None, ROWS2]),
    "encode_with_coefs/null_coefs_empty": ("vga_gcadpcm_encode_with_coefs_batch", [None, 2, 100, 0, None, None, None, None]),
    "encode_with_coefs/negative_count_empty": ("vga_gcadpcm_encode_with_coefs_batch", [None, -1, 100, 0, A, None, None, None]),
    "encode_batch/negative_and_null_rows": ("vga_gcadpcm_encode_batch", [None, 2, -1, 0, 0, None, None]),
    "encode_batch/negative_count_and_null_rows": ("vga_gcadpcm_encode_batch", [None, -1, 100, 0, 0, None, None]),
    "encode_batch/null_rows_and_null_out": ("vga_gcadpcm_encode_batch", [None, 2, 100, 0, 0, None, None]),
    "encode_batch/null_row_and_null_out_row": ("vga_gcadpcm_encode_batch", [NULLROW, 2, 100, 0, 0, A, NULLROW]),
    "encode_batch/null_out_and_null_coefs": ("vga_gcadpcm_encode_batch", [ROWS2, 2, 100, 0, 0, None, None]),
    "encode_batch/null_coefs": ("vga_gcadpcm_encode_batch", [ROWS2, 2, 100, 0, 0, None, ROWS2]),
    "encode_batch/null_coefs_empty": ("vga_gcadpcm_encode_batch", [None, 2, 0, 0, 0, None, None]),
    "encode_batch/negative_count_empty": ("vga_gcadpcm_encode_batch", [None, -1, 0, 0, 0, A, None]),
    "decode_batch/negative_and_null_rows": ("vga_gcadpcm_decode_batch", [None, None, 2, -1, None, None, None]),
    "decode_batch/negative_count_and_null_rows": ("vga_gcadpcm_decode_batch", [None, None, -1, 100, None, None, None]),
    "decode_batch/null_rows_and_null_coefs": ("vga_gcadpcm_decode_batch", [None, None, 2, 100, None, None, None]),
    "decode_batch/null_row_and_null_out": ("vga_gcadpcm_decode_batch", [NULLROW, A, 2, 100, None, None, None]),
    "decode_batch/null_out_and_null_coefs": ("vga_gcadpcm_decode_batch", [ROWS2, None, 2, 100, None, None, None]),
    "decode_batch/null_out_row": ("vga_gcadpcm_decode_batch", [ROWS2, A, 2, 100, None, None, NULLROW]),
    "decode_batch/null_coefs": ("vga_gcadpcm_decode_batch", [ROWS2, None, 2, 100, None, None, ROWS2]),
    "decode_batch/null_coefs_empty": ("vga_gcadpcm_decode_batch", [None, None, 2, 0, None, None, None]),
    "decode_batch/negative_count_empty": ("vga_gcadpcm_decode_batch", [None, A, -1, 0, None, None, None]),
    # the ragged host batches
    "encode_v/null_out_and_negative_count": ("vga_gcadpcm_encode_batch_v", [None, None, 2, None, None, None, None]),
    "encode_v/negative_count": ("vga_gcadpcm_encode_batch_v", [None, None, -1, None, None, None, None]),
    "encode_v/null_counts_and_null_rows": ("vga_gcadpcm_encode_batch_v", [None, None, 2, None, None, None, ROWS2]),
    "encode_v/negative_sample_count_and_null_row": ("vga_gcadpcm_encode_batch_v", [NULLROW, ("ints", 100, -5), 2, None, None, None, ROWS2]),
    "encode_v/null_rows_and_null_coefs": ("vga_gcadpcm_encode_batch_v", [None, ("ints", 100, 50), 2, None, None, None, ROWS2]),
    "encode_v/null_row_and_null_out_row": ("vga_gcadpcm_encode_batch_v", [NULLROW, ("ints", 100, 50), 2, None, None, A, NULLROW]),
    "encode_v/null_out_row_and_null_coefs": ("vga_gcadpcm_encode_batch_v", [ROWS2, ("ints", 100, 50), 2, None, None, None, NULLROW]),
    "encode_v/null_coefs": ("vga_gcadpcm_encode_batch_v", [ROWS2, ("ints", 100, 50), 2, None, None, None, ROWS2]),
    "encode_v/null_coefs_sorted": ("vga_gcadpcm_encode_batch_v", [ROWS2, ("ints", 50, 100), 2, None, None, None, ROWS2]),
    "coefs_v/negative_count": ("vga_gcadpcm_calculate_coefficients_batch_v", [None, None, -3, None]),
    "coefs_v/null_counts": ("vga_gcadpcm_calculate_coefficients_batch_v", [ROWS2, None, 2, A]),
    "coefs_v/null_row_and_null_coefs": ("vga_gcadpcm_calculate_coefficients_batch_v", [NULLROW, ("ints", 100, 50), 2, None]),
    "coefs_v/null_coefs": ("vga_gcadpcm_calculate_coefficients_batch_v", [ROWS2, ("ints", 100, 50), 2, None]),
    "encode_with_coefs_v/null_out": ("vga_gcadpcm_encode_with_coefs_batch_v", [ROWS2, ("ints", 100, 50), 2, A, None, None, None]),
    "encode_with_coefs_v/negative_sample_count": ("vga_gcadpcm_encode_with_coefs_batch_v", [ROWS2, ("ints", -1, 50), 2, None, None, None, ROWS2]),
    "encode_with_coefs_v/null_out_row_and_null_coefs": ("vga_gcadpcm_encode_with_coefs_batch_v", [ROWS2, ("ints", 100, 50), 2, None, None, None, NULLROW]),
    "encode_with_coefs_v/null_coefs": ("vga_gcadpcm_encode_with_coefs_batch_v", [ROWS2, ("ints", 100, 50), 2, None, None, None, ROWS2]),
    "decode_v/negative_count": ("vga_gcadpcm_decode_batch_v", [None, None, None, -1, None, None, None]),
    "decode_v/null_counts": ("vga_gcadpcm_decode_batch_v", [ROWS2, A, None, 2, None, None, ROWS2]),
    "decode_v/negative_sample_count_and_null_rows": ("vga_gcadpcm_decode_batch_v", [None, None, ("ints", 100, -1), 2, None, None, None]),
    "decode_v/null_rows": ("vga_gcadpcm_decode_batch_v", [None, A, ("ints", 100, 50), 2, None, None, ROWS2]),
    "decode_v/null_row_and_null_out": ("vga_gcadpcm_decode_batch_v", [NULLROW, A, ("ints", 100, 50), 2, None, None, None]),
    "decode_v/null_out_row_and_null_coefs": ("vga_gcadpcm_decode_batch_v", [ROWS2, None, ("ints", 100, 50), 2, None, None, NULLROW]),
    "decode_v/null_coefs": ("vga_gcadpcm_decode_batch_v", [ROWS2, None, ("ints", 100, 50), 2, None, None, ROWS2]),
    "decode_v/null_coefs_sorted": ("vga_gcadpcm_decode_batch_v", [ROWS2, None, ("ints", 50, 100), 2, None, None, ROWS2]),
    # the ragged object
    "ragged_create/null_output": ("vga_gcadpcm_ragged_create", [("ints", 100, 50), 2, None]),
    "ragged_create/negative_count": ("vga_gcadpcm_ragged_create", [None, -1, A]),
}
# the ragged object's creator writes *out = NULL before it tests the rest: its output is a real pointer-sized cell
REAL_OUTPUT = {"ragged_create/negative_count": 2}


def _structs():
    from vgaudio_amd import _lib
    return {"chan": _lib.GcChannelParamsC, "dsp": _lib.DspParamsC}


def marshal(value, argtype, keep):
    """one argument of a refused call as ctypes takes it; `keep` holds what must outlive the call"""
    if isinstance(value, tuple):
        kind, items = value[0], value[1:]
        if kind == "rows":
            obj = (C.c_void_p * len(items))(*items)
        elif kind == "ints":
            obj = (C.c_int * len(items))(*items)
        else:
            obj = _structs()[kind](*items)
        keep.append(obj)
        return C.cast(C.pointer(obj), argtype)
    if value is None or not hasattr(argtype, "contents") and argtype is not C.c_void_p:
        return value
    return C.cast(C.c_void_p(value), argtype)


def call_refused(L, signatures, name):
    """(code, message) of one refused call; the message before it is a known one, for a refusal that sets none"""
    fn_name, args = REFUSED_CALLS[name]
    restype, argtypes = signatures[fn_name]
    fn = getattr(L, fn_name)
    fn.restype, fn.argtypes = restype, argtypes
    L.vga_last_error.restype = C.c_char_p
    L.vga_dsp_layout_for.restype, L.vga_dsp_layout_for.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_void_p]
    assert L.vga_dsp_layout_for(None, 1, None) != 0            # leaves "null argument"
    keep = []
    args = list(args)
    if name in REAL_OUTPUT:
        cell = C.c_void_p(0)
        keep.append(cell)
        args[REAL_OUTPUT[name]] = C.addressof(cell)
    rc = fn(*[marshal(v, t, keep) for v, t in zip(args, argtypes)])
    return rc, L.vga_last_error().decode()


def layout_call(fn, params_type, layout_type, case):
    """(code, message, the output's bytes) of one layout case; the output starts as 0x5A bytes"""
    params, nch, null = case
    p, out = params_type(*params), layout_type()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    args = [None if null == 1 else C.byref(p), None if null == 2 else C.byref(out)]
    rc = fn(args[0], args[1]) if params_type is _structs()["chan"] else fn(args[0], nch, args[1])
    return rc, bytes(out)


def record(library):
    sys.path.insert(0, os.path.join(HERE, ".."))
    from vgaudio_amd import _lib
    L = C.CDLL(library)
    out = {}
    for name in REFUSED_CALLS:
        rc, message = call_refused(L, _lib.SIGNATURES, name)
        # a call that got as far as the device is not a refusal of an argument test: it must not be in this table
        assert rc not in (0, _lib.VGA_ERR_DEVICE), (name, rc, message)
        out[name] = [rc, message]
    L.vga_gcadpcm_channel_layout_for.argtypes = [C.c_void_p, C.c_void_p]
    for kind, cases, fn, types in (("channel", CHANNEL_CASES, L.vga_gcadpcm_channel_layout_for, (_lib.GcChannelParamsC, _lib.GcChannelLayoutC)),
                                   ("dsp", DSP_CASES, L.vga_dsp_layout_for, (_lib.DspParamsC, _lib.DspLayoutC))):
        for name, case in cases.items():
            rc, layout = layout_call(fn, *types, case)
            assert (rc != 0) == name.startswith("refused_"), (kind, name, rc)
            if rc:
                out["layout/%s/%s" % (kind, name)] = [rc, L.vga_last_error().decode(), layout.hex()]
    with open(RECORD, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(out), "refusals ->", RECORD)


if __name__ == "__main__":
    default = os.path.join(HERE, "..", "vgaudio_amd", "libvgaudio_hip.so")
    record(sys.argv[sys.argv.index("--library") + 1] if "--library" in sys.argv else default)

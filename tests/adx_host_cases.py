"""The case tables of tests/test_adx_host_layer.py (test code only), and the generator of what is recorded in
tests/golden/adx_host_refusals.json:

    python tests/adx_host_cases.py [--library PATH/libvgaudio_hip.so]

runs every refused call below, and the pure size and conversion functions over the inputs below, on a build of the PARENT
of the change that moved the CRI ADX host layer into csrc/adx_host.hpp, and writes each call's code and message and each
function's values: the yardstick is that library, not the moved code.  Every call of REFUSED_CALLS is one an argument test
refuses before anything reaches the device, so the table needs no GPU; data pointers are never dereferenced on those paths and
are dummy addresses, the row, count and parameter arrays are real.  ACCEPTED_CALLS pass every argument test: they would go on
to the device with those dummy addresses, so they are never made -- only the header's checks see them."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(HERE, "golden", "adx_host_refusals.json")

# ---- arguments: an int is itself (a dummy address where the parameter is a pointer), None a null pointer, ("rows", ...) an
# array of pointers, ("ints", ...) an int array, ("adx", {...}, ...) an array of vga_adx_params, each the defaults
# (vga_adx_default_params: 48000 Hz, high-pass 500, 18-byte frames, version 4, no padding, type 3) with the named fields set
A, B, D = 0x100000, 0x200000, 0x300000          # aligned dummy addresses
ROWS2, NULL0, NULL1 = ("rows", A, B), ("rows", None, B), ("rows", A, None)
ROWS3, NULL2 = ("rows", A, B, D), ("rows", A, B, None)
FIELDS = ("sample_rate", "highpass_frequency", "frame_size", "version", "history", "padding", "type", "filter")
DEFAULTS = dict(zip(FIELDS, (48000, 500, 18, 4, 0, 0, 3, 0)))


def P(**kw):
    return ("adx", kw)


OK, V3, PAD10, PAD40, FIXED3 = P(), P(version=3), P(padding=10), P(padding=40), P(type=2, filter=3, sample_rate=0)
# every branch of adx::validate, in its order, after the null pointer
BAD = {
    "frame_size_2": P(frame_size=2), "frame_size_odd": P(frame_size=17), "frame_size_256": P(frame_size=256),
    "type_5": P(type=5), "type_1": P(type=1), "fixed_filter_4": P(type=2, filter=4), "fixed_filter_negative": P(type=2, filter=-1),
    "negative_padding": P(padding=-1), "sample_rate_0": P(sample_rate=0), "sample_rate_negative": P(type=4, sample_rate=-8000),
}
TWO_BAD = P(frame_size=17, type=5, padding=-1)         # the frame size is asked first


def PP(*sets):
    """an array of parameter sets, one per channel of a ragged call"""
    return ("adx",) + tuple(s[1] for s in sets)


def spf(p):
    return (dict(DEFAULTS, **p[1])["frame_size"] - 2) * 2


def reads(n, p):
    """bytes the decoder reads for n samples: the frames before the one the padding ends in, then ceil(n / spf) frames"""
    q = dict(DEFAULTS, **p[1])
    return (q["padding"] // spf(p) + -(-n // spf(p))) * q["frame_size"]


assert (reads(1000, OK), reads(1000, PAD40), reads(64, P(frame_size=34))) == (576, 594, 34)

REFUSED_CALLS = {}
ACCEPTED_CALLS = {}


def refused(name, fn, args):
    assert name not in REFUSED_CALLS and name not in ACCEPTED_CALLS
    REFUSED_CALLS[name] = (fn, args)


def accepted(name, fn, args):
    assert name not in REFUSED_CALLS and name not in ACCEPTED_CALLS
    ACCEPTED_CALLS[name] = (fn, args)


# ---- vga_adx_encoded_byte_count(pcm_length, p) and vga_adx_calculate_coefficients(highpass, sample_rate, coefs_out)
refused("size/null_params", "vga_adx_encoded_byte_count", [100, None])
for _k, _p in BAD.items():
    refused("size/" + _k, "vga_adx_encoded_byte_count", [100, _p])
refused("size/negative_length", "vga_adx_encoded_byte_count", [-1, OK])                 # (sets no message)
refused("size/two_bad_fields", "vga_adx_encoded_byte_count", [100, TWO_BAD])
refused("size/bad_params_and_negative_length", "vga_adx_encoded_byte_count", [-1, BAD["type_5"]])
refused("size/null_params_and_negative_length", "vga_adx_encoded_byte_count", [-1, None])
refused("size/fixed_filter_and_negative_padding", "vga_adx_encoded_byte_count", [100, P(type=2, filter=7, padding=-1)])
refused("coefs/null_output", "vga_adx_calculate_coefficients", [500, 48000, None])
refused("coefs/sample_rate_0", "vga_adx_calculate_coefficients", [500, 0, A])
refused("coefs/sample_rate_negative", "vga_adx_calculate_coefficients", [500, -1, A])
refused("coefs/null_output_and_sample_rate_0", "vga_adx_calculate_coefficients", [500, 0, None])       # (one test of two conditions:
refused("coefs/null_output_and_sample_rate_negative", "vga_adx_calculate_coefficients", [0, -8000, None])   # there is no order to pin)

# ---- vga_adx_encode_device(d_pcm, pcm_pitch, nch, pcm_length, p, d_out, out_pitch, d_history_out, stream); 1000 samples
# of 18-byte frames are 32 frames = 576 bytes
ENC = "vga_adx_encode_device"
refused("encode_device/null_params", ENC, [A, 1000, 2, 1000, None, B, 576, None, None])
for _k, _p in BAD.items():
    refused("encode_device/" + _k, ENC, [A, 1000, 2, 1000, _p, B, 576, None, None])
refused("encode_device/negative_channels", ENC, [A, 1000, -1, 1000, OK, B, 576, None, None])
refused("encode_device/negative_length", ENC, [A, 1000, 2, -1, OK, B, 576, None, None])
refused("encode_device/empty_pcm", ENC, [A, 8, 2, 0, OK, B, 16, None, None])
accepted("encode_device/empty_pcm_version_3", ENC, [A, 8, 2, 0, V3, B, 16, None, None])
accepted("encode_device/empty_pcm_padding_10", ENC, [A, 8, 2, 0, PAD10, B, 18, None, None])
accepted("encode_device/empty_pcm_no_channels", ENC, [A, 8, 0, 0, OK, B, 16, None, None])
refused("encode_device/pcm_pitch_short", ENC, [A, 999, 2, 1000, OK, B, 576, None, None])
refused("encode_device/out_pitch_short", ENC, [A, 1000, 2, 1000, OK, B, 574, None, None])
refused("encode_device/out_pitch_odd", ENC, [A, 1000, 2, 1000, OK, B, 577, None, None])
refused("encode_device/out_odd", ENC, [A, 1000, 2, 1000, OK, B + 1, 576, None, None])
refused("encode_device/out_pitch_short_with_padding", ENC, [A, 1000, 2, 1000, PAD40, B, 576, None, None])   # 1040 samples: 33 frames
accepted("encode_device/tight", ENC, [A, 1000, 2, 1000, OK, B, 576, None, None])
accepted("encode_device/tight_with_padding", ENC, [A, 1000, 2, 1000, PAD40, B, 594, None, None])
accepted("encode_device/fixed_filter_3_without_a_sample_rate", ENC, [A, 1000, 2, 1000, FIXED3, B, 576, None, None])
refused("encode_device/bad_params_and_negative", ENC, [A, 1000, -1, -1, BAD["frame_size_odd"], B, 576, None, None])
refused("encode_device/negative_and_empty_pcm", ENC, [A, 8, -1, 0, OK, B + 1, 16, None, None])
refused("encode_device/empty_pcm_and_bad_pitch", ENC, [A, 8, 2, 0, OK, B + 1, 15, None, None])
refused("encode_device/null_params_and_negative", ENC, [A, 1000, 2, -1, None, B, 576, None, None])

# ---- vga_adx_decode_device(d_adpcm, in_pitch, adpcm_length, nch, sample_count, p, d_pcm, pcm_pitch, d_status, stream)
DEC = "vga_adx_decode_device"
refused("decode_device/null_params", DEC, [A, 576, 576, 2, 1000, None, B, 1000, D, None])
for _k, _p in BAD.items():
    refused("decode_device/" + _k, DEC, [A, 576, 576, 2, 1000, _p, B, 1000, D, None])
refused("decode_device/negative_channels", DEC, [A, 576, 576, -1, 1000, OK, B, 1000, D, None])
refused("decode_device/negative_samples", DEC, [A, 576, 576, 2, -1, OK, B, 1000, D, None])
refused("decode_device/negative_bytes", DEC, [A, 576, -1, 2, 1000, OK, B, 1000, D, None])
refused("decode_device/one_byte_short", DEC, [A, 576, 575, 2, 1000, OK, B, 1000, D, None])
refused("decode_device/one_byte_short_with_padding", DEC, [A, 600, 593, 2, 1000, PAD40, B, 1000, D, None])
refused("decode_device/one_byte_short_frame_34", DEC, [A, 40, 33, 2, 64, P(frame_size=34), B, 64, D, None])
accepted("decode_device/exactly_long_enough", DEC, [A, 576, 576, 2, 1000, OK, B, 1000, D, None])
accepted("decode_device/exactly_long_enough_with_padding", DEC, [A, 600, 594, 2, 1000, PAD40, B, 1000, D, None])
accepted("decode_device/exactly_long_enough_frame_34", DEC, [A, 40, 34, 2, 64, P(frame_size=34), B, 64, D, None])
accepted("decode_device/no_samples_of_no_bytes", DEC, [A, 0, 0, 2, 0, OK, B, 0, D, None])
refused("decode_device/in_pitch_short", DEC, [A, 575, 576, 2, 1000, OK, B, 1000, D, None])
refused("decode_device/pcm_pitch_short", DEC, [A, 576, 576, 2, 1000, OK, B, 999, D, None])
refused("decode_device/bad_params_and_negative", DEC, [A, 576, -1, 2, 1000, BAD["negative_padding"], B, 1000, D, None])
refused("decode_device/negative_and_short", DEC, [A, 576, 10, 2, -5, OK, B, 1000, D, None])
refused("decode_device/null_params_and_negative", DEC, [A, 576, 576, -2, 1000, None, B, 1000, D, None])
refused("decode_device/short_and_pitches_short", DEC, [A, 100, 570, 2, 1000, OK, B, 10, D, None])

# ---- vga_adx_encode_batch(pcm, nch, pcm_length, p, out, history_out)
ENCB = "vga_adx_encode_batch"
refused("encode_batch/null_params", ENCB, [ROWS2, 2, 1000, None, ROWS2, None])
for _k, _p in BAD.items():
    refused("encode_batch/" + _k, ENCB, [ROWS2, 2, 1000, _p, ROWS2, None])
refused("encode_batch/negative_channels", ENCB, [ROWS2, -2, 1000, OK, ROWS2, None])
refused("encode_batch/negative_length", ENCB, [ROWS2, 2, -1, OK, ROWS2, None])
refused("encode_batch/null_pcm_array", ENCB, [None, 2, 1000, OK, ROWS2, None])
refused("encode_batch/null_out_array", ENCB, [ROWS2, 2, 1000, OK, None, None])
refused("encode_batch/null_pcm_row_0", ENCB, [NULL0, 2, 1000, OK, ROWS2, None])
refused("encode_batch/null_pcm_row_last", ENCB, [NULL2, 3, 1000, OK, ROWS3, None])
refused("encode_batch/null_out_row_0", ENCB, [ROWS2, 2, 1000, OK, NULL0, None])
refused("encode_batch/null_out_row_last", ENCB, [ROWS3, 3, 1000, OK, NULL2, None])
refused("encode_batch/null_out_row_of_an_empty_pcm", ENCB, [NULL0, 2, 0, PAD10, NULL1, None])    # (a null PCM row of no samples is none)
refused("encode_batch/empty_pcm", ENCB, [ROWS2, 2, 0, OK, ROWS2, None])
refused("encode_batch/empty_pcm_null_rows", ENCB, [NULL0, 2, 0, OK, ROWS2, None])
accepted("encode_batch/empty_pcm_version_3", ENCB, [NULL0, 2, 0, V3, ROWS2, None])
accepted("encode_batch/empty_pcm_padding_40", ENCB, [ROWS2, 2, 0, PAD40, ROWS2, None])
accepted("encode_batch/three_rows", ENCB, [ROWS3, 3, 1000, OK, ROWS3, A])
refused("encode_batch/bad_params_and_null_array", ENCB, [None, 2, 1000, BAD["type_1"], None, None])
refused("encode_batch/negative_and_null_array", ENCB, [None, 2, -1, OK, None, None])
refused("encode_batch/null_array_and_empty_pcm", ENCB, [ROWS2, 2, 0, OK, None, None])
refused("encode_batch/null_out_row_and_empty_pcm", ENCB, [ROWS2, 2, 0, OK, NULL1, None])

# ---- vga_adx_decode_batch(adpcm, adpcm_length, nch, sample_count, p, pcm_out)
DECB = "vga_adx_decode_batch"
refused("decode_batch/null_params", DECB, [ROWS2, 576, 2, 1000, None, ROWS2])
for _k, _p in BAD.items():
    refused("decode_batch/" + _k, DECB, [ROWS2, 576, 2, 1000, _p, ROWS2])
refused("decode_batch/negative_channels", DECB, [ROWS2, 576, -1, 1000, OK, ROWS2])
refused("decode_batch/negative_samples", DECB, [ROWS2, 576, 2, -1, OK, ROWS2])
refused("decode_batch/negative_bytes", DECB, [ROWS2, -576, 2, 1000, OK, ROWS2])
refused("decode_batch/null_adpcm_array", DECB, [None, 576, 2, 1000, OK, ROWS2])
refused("decode_batch/null_out_array", DECB, [ROWS2, 576, 2, 1000, OK, None])
refused("decode_batch/null_adpcm_row_0", DECB, [NULL0, 576, 2, 1000, OK, ROWS2])
refused("decode_batch/null_adpcm_row_last", DECB, [NULL2, 576, 3, 1000, OK, ROWS3])
refused("decode_batch/null_out_row_0", DECB, [ROWS2, 576, 2, 1000, OK, NULL0])
refused("decode_batch/null_out_row_last", DECB, [ROWS3, 576, 3, 1000, OK, NULL2])
refused("decode_batch/one_byte_short", DECB, [ROWS2, 575, 2, 1000, OK, ROWS2])
refused("decode_batch/one_byte_short_with_padding", DECB, [ROWS2, 593, 2, 1000, PAD40, ROWS2])
accepted("decode_batch/exactly_long_enough", DECB, [ROWS3, 576, 3, 1000, OK, ROWS3])
accepted("decode_batch/exactly_long_enough_with_padding", DECB, [ROWS2, 594, 2, 1000, PAD40, ROWS2])
accepted("decode_batch/no_samples_null_arrays", DECB, [None, 0, 2, 0, OK, None])
refused("decode_batch/bad_params_and_null_array", DECB, [None, 576, 2, 1000, BAD["sample_rate_0"], None])
refused("decode_batch/negative_and_null_array", DECB, [None, 576, 2, -1, OK, None])
refused("decode_batch/null_row_and_short", DECB, [NULL1, 10, 2, 1000, OK, ROWS2])
refused("decode_batch/null_array_and_short", DECB, [None, 10, 2, 1000, OK, ROWS2])

# ---- vga_adx_encode_batch_v(pcm, pcm_lengths, nch, params, out, history_out)
ENCV = "vga_adx_encode_batch_v"
LEN2, LEN3 = ("ints", 1000, 50), ("ints", 1000, 50, 7)
refused("encode_v/negative_channels", ENCV, [ROWS2, LEN2, -1, PP(OK, OK), ROWS2, None])
refused("encode_v/null_pcm_array", ENCV, [None, LEN2, 2, PP(OK, OK), ROWS2, None])
refused("encode_v/null_lengths", ENCV, [ROWS2, None, 2, PP(OK, OK), ROWS2, None])
refused("encode_v/null_params", ENCV, [ROWS2, LEN2, 2, None, ROWS2, None])
refused("encode_v/null_out_array", ENCV, [ROWS2, LEN2, 2, PP(OK, OK), None, None])
for _k, _p in BAD.items():
    refused("encode_v/channel_1_" + _k, ENCV, [ROWS2, LEN2, 2, PP(V3, _p), ROWS2, None])
refused("encode_v/channel_0_bad_params", ENCV, [ROWS2, LEN2, 2, PP(BAD["type_5"], OK), ROWS2, None])
refused("encode_v/channel_1_negative_length", ENCV, [ROWS2, ("ints", 1000, -50), 2, PP(OK, OK), ROWS2, None])
refused("encode_v/channel_1_empty_pcm", ENCV, [ROWS2, ("ints", 1000, 0), 2, PP(OK, OK), ROWS2, None])
refused("encode_v/channel_2_empty_pcm_of_its_own_version", ENCV, [ROWS3, ("ints", 0, 0, 0), 3, PP(V3, PAD10, OK), ROWS3, None])
accepted("encode_v/empty_pcm_version_3_and_padding", ENCV, [NULL0, ("ints", 0, 0), 2, PP(V3, PAD40), ROWS2, None])
refused("encode_v/null_pcm_row_0", ENCV, [NULL0, LEN2, 2, PP(OK, OK), ROWS2, None])
refused("encode_v/null_pcm_row_last", ENCV, [NULL2, LEN3, 3, PP(OK, V3, PAD10), ROWS3, None])
refused("encode_v/null_out_row_0", ENCV, [ROWS2, LEN2, 2, PP(OK, OK), NULL0, None])
refused("encode_v/null_out_row_last", ENCV, [ROWS3, LEN3, 3, PP(OK, V3, PAD10), NULL2, None])
refused("encode_v/null_out_row_of_an_empty_pcm", ENCV, [NULL2, ("ints", 1000, 50, 0), 3, PP(OK, OK, PAD10), NULL2, None])
accepted("encode_v/three_channels", ENCV, [ROWS3, LEN3, 3, PP(OK, FIXED3, P(frame_size=34, padding=40)), ROWS3, A])
accepted("encode_v/no_channels_null_arrays", ENCV, [None, None, 0, None, None, None])
refused("encode_v/negative_channels_and_null_arrays", ENCV, [None, None, -3, None, None, None])
refused("encode_v/null_row_0_and_bad_params_1", ENCV, [NULL0, LEN2, 2, PP(OK, BAD["type_5"]), ROWS2, None])
refused("encode_v/negative_length_0_and_bad_params_1", ENCV, [ROWS2, ("ints", -1, 50), 2, PP(OK, BAD["negative_padding"]), ROWS2, None])
refused("encode_v/bad_params_and_negative_length_in_one_channel", ENCV, [ROWS2, ("ints", 1000, -1), 2, PP(OK, BAD["frame_size_2"]), ROWS2, None])
refused("encode_v/negative_length_and_null_row_in_one_channel", ENCV, [NULL1, ("ints", 1000, -1), 2, PP(OK, OK), NULL1, None])
refused("encode_v/empty_pcm_and_null_out_row_in_one_channel", ENCV, [ROWS2, ("ints", 1000, 0), 2, PP(OK, OK), NULL1, None])

# ---- vga_adx_decode_batch_v(adpcm, adpcm_lengths, nch, sample_counts, params, pcm_out)
DECV = "vga_adx_decode_batch_v"
BYTES2, BYTES3 = ("ints", 576, 36), ("ints", 576, 36, 18)
refused("decode_v/negative_channels", DECV, [ROWS2, BYTES2, -1, LEN2, PP(OK, OK), ROWS2])
refused("decode_v/null_adpcm_array", DECV, [None, BYTES2, 2, LEN2, PP(OK, OK), ROWS2])
refused("decode_v/null_byte_counts", DECV, [ROWS2, None, 2, LEN2, PP(OK, OK), ROWS2])
refused("decode_v/null_sample_counts", DECV, [ROWS2, BYTES2, 2, None, PP(OK, OK), ROWS2])
refused("decode_v/null_params", DECV, [ROWS2, BYTES2, 2, LEN2, None, ROWS2])
refused("decode_v/null_out_array", DECV, [ROWS2, BYTES2, 2, LEN2, PP(OK, OK), None])
for _k, _p in BAD.items():
    refused("decode_v/channel_1_" + _k, DECV, [ROWS2, BYTES2, 2, LEN2, PP(V3, _p), ROWS2])
refused("decode_v/channel_0_bad_params", DECV, [ROWS2, BYTES2, 2, LEN2, PP(BAD["frame_size_256"], OK), ROWS2])
refused("decode_v/channel_1_negative_samples", DECV, [ROWS2, BYTES2, 2, ("ints", 1000, -50), PP(OK, OK), ROWS2])
refused("decode_v/channel_1_negative_bytes", DECV, [ROWS2, ("ints", 576, -36), 2, LEN2, PP(OK, OK), ROWS2])
refused("decode_v/channel_1_one_byte_short", DECV, [ROWS2, ("ints", 576, 35), 2, LEN2, PP(OK, OK), ROWS2])
refused("decode_v/channel_2_one_byte_short_with_padding", DECV, [ROWS3, ("ints", 576, 36, 35), 3, LEN3, PP(OK, OK, PAD40), ROWS3])
accepted("decode_v/exactly_long_enough", DECV, [ROWS3, ("ints", 576, 36, 36), 3, LEN3, PP(OK, V3, PAD40), ROWS3])
accepted("decode_v/no_samples_read_nothing", DECV, [NULL1, ("ints", 576, 0), 2, ("ints", 1000, 0), PP(OK, PAD40), NULL1])
refused("decode_v/null_adpcm_row_0", DECV, [NULL0, BYTES2, 2, LEN2, PP(OK, OK), ROWS2])
refused("decode_v/null_adpcm_row_last", DECV, [NULL2, BYTES3, 3, LEN3, PP(OK, OK, OK), ROWS3])
refused("decode_v/null_out_row_0", DECV, [ROWS2, BYTES2, 2, LEN2, PP(OK, OK), NULL0])
refused("decode_v/null_out_row_last", DECV, [ROWS3, BYTES3, 3, LEN3, PP(OK, OK, OK), NULL2])
accepted("decode_v/no_channels_null_arrays", DECV, [None, None, 0, None, None, None])
refused("decode_v/negative_channels_and_null_arrays", DECV, [None, None, -1, None, None, None])
refused("decode_v/short_0_and_bad_params_1", DECV, [ROWS2, ("ints", 575, 36), 2, LEN2, PP(OK, BAD["type_5"]), ROWS2])
refused("decode_v/negative_and_short_in_one_channel", DECV, [ROWS2, ("ints", 576, -1), 2, ("ints", 1000, 5000), PP(OK, OK), ROWS2])
refused("decode_v/short_and_null_row_in_one_channel", DECV, [NULL1, ("ints", 576, 35), 2, LEN2, PP(OK, OK), ROWS2])
refused("decode_v/null_row_0_and_short_1", DECV, [ROWS2, ("ints", 576, 35), 2, LEN2, PP(OK, OK), NULL0])

ENTRY_POINTS = ["vga_adx_encoded_byte_count", "vga_adx_calculate_coefficients", ENC, DEC, ENCB, DECB, ENCV, DECV]

# ---- the pure functions' accepted values
NEAR_2_31 = [2**31 - 1 - k for k in range(41)]
SIZE_LENGTHS = list(range(201)) + NEAR_2_31
SIZE_SETS = {
    "frame_4": P(frame_size=4), "frame_18": OK, "frame_34_padding_10": P(frame_size=34, padding=10),
    "frame_254_padding_40": P(frame_size=254, padding=40), "frame_18_padding_40": PAD40,
    "padding_wraps": P(padding=2**31 - 100),                   # pcm_length + padding wraps from pcm_length 100 on
}
CONVERSIONS = ["vga_adx_nibble_count_to_sample_count", "vga_adx_sample_count_to_nibble_count", "vga_adx_sample_count_to_byte_count"]
CONVERSION_INPUTS = list(range(4098)) + NEAR_2_31[::-1]
CONVERSION_FRAME_SIZES = [4, 18, 254]


def params_struct(fields):
    from vgaudio_amd import _lib
    p = _lib.AdxParams()
    for k, v in dict(DEFAULTS, **fields).items():
        setattr(p, k, v)
    return p


def marshal(value, argtype, keep):
    """one argument of a call as ctypes takes it; `keep` holds what must outlive the call"""
    if isinstance(value, tuple):
        kind, items = value[0], value[1:]
        if kind == "rows":
            obj = (C.c_void_p * len(items))(*items)
        elif kind == "ints":
            obj = (C.c_int * len(items))(*items)
        else:
            from vgaudio_amd import _lib
            obj = (_lib.AdxParams * len(items))(*[params_struct(f) for f in items])
        keep.append(obj)
        return C.cast(C.pointer(obj), argtype)
    if value is None or not hasattr(argtype, "contents") and argtype is not C.c_void_p:
        return value
    return C.cast(C.c_void_p(value), argtype)


KNOWN_MESSAGE = "bad arguments"


def call(L, prefix, signatures, fn_name, args):
    """(code, message) of one call of L's <prefix><name without vga_adx_>; the message before it is KNOWN_MESSAGE, for a
    refusal that sets none"""
    restype, argtypes = signatures[fn_name]
    fn = getattr(L, prefix + fn_name[len("vga_adx_"):])
    fn.restype, fn.argtypes = restype, argtypes
    first = getattr(L, prefix + "calculate_coefficients")
    first.restype, first.argtypes = signatures["vga_adx_calculate_coefficients"]
    last_error = getattr(L, "vga_last_error" if prefix == "vga_adx_" else prefix + "last_error")
    last_error.restype = C.c_char_p
    assert first(0, 0, None) != 0 and last_error().decode() == KNOWN_MESSAGE
    keep = []
    rc = fn(*[marshal(v, t, keep) for v, t in zip(args, argtypes)])
    return rc, last_error().decode()


def sizes_of(byte_count, fields):
    p = params_struct(fields)
    return [byte_count(n, C.byref(p)) for n in SIZE_LENGTHS]


def record(library):
    sys.path.insert(0, os.path.join(HERE, ".."))
    from vgaudio_amd import _lib
    L = C.CDLL(library)
    out = {"refusals": {}, "encoded_byte_count": {}, "conversions": {}}
    for name, (fn, args) in REFUSED_CALLS.items():
        rc, message = call(L, "vga_adx_", _lib.SIGNATURES, fn, args)
        # a call that got as far as the device is not a refusal of an argument test: it must not be in this table
        assert rc not in (0, _lib.VGA_ERR_DEVICE), (name, rc, message)
        out["refusals"][name] = [rc, message]
    L.vga_adx_encoded_byte_count.restype, L.vga_adx_encoded_byte_count.argtypes = C.c_int, [C.c_int, C.c_void_p]
    for name, p in SIZE_SETS.items():
        out["encoded_byte_count"][name] = sizes_of(L.vga_adx_encoded_byte_count, p[1])
    for fn in CONVERSIONS:
        f = getattr(L, fn)
        f.restype, f.argtypes = C.c_int, [C.c_int, C.c_int]
        for fs in CONVERSION_FRAME_SIZES:
            out["conversions"]["%s/%d" % (fn, fs)] = [f(n, fs) for n in CONVERSION_INPUTS]
    with open(RECORD, "w") as f:                                # one table entry per line
        f.write("{\n" + ",\n".join('"%s": {\n%s\n}' % (k, ",\n".join("%s: %s" % (json.dumps(n), json.dumps(v, separators=(",", ":")))
                                                                      for n, v in sorted(table.items())))
                                   for k, table in sorted(out.items())) + "\n}\n")
    print(len(out["refusals"]), "refusals,", len(out["encoded_byte_count"]), "size sets,", len(out["conversions"]), "conversion tables ->", RECORD)


if __name__ == "__main__":
    default = os.path.join(HERE, "..", "vgaudio_amd", "libvgaudio_hip.so")
    record(sys.argv[sys.argv.index("--library") + 1] if "--library" in sys.argv else default)

"""Inputs that send the CRI HCA encoder down the ways its frames rarely go (tables and generators only; the CPU tests in
test_hca_encoder_paths_host.py and the GPU tests in test_gpu_hca_encoder_paths.py both import this file).

CriHcaEncoder.EncodeFrame makes a handful of data-dependent decisions, and noise, tones and the synthetic bench channels
take nearly all of them the same way: over the 1899 frames of the older HCA tests no channel header wrote its scale
factors raw, no intensity index reached its bound of 13, no HFR group scale took 1 / average, and 12 frames in all dropped
bands.  The kernels restate each of those ways as separate code.  Every CASE below is a small seeded signal that takes one
or more of them in at least half of its frames (or of the units the counter counts), which the oracle's path counters
(oracle.h: vgo_hca_encode_paths, po.hca_encode_paths()) confirm in the `reach` condition: a condition that fails is a
test failure, never a skip.  RECORDED at the end of the file lists the counters of every case.

Paths (PATHS) and the reference lines they stand for (CriHcaEncoder.cs unless named):
  raw_scale_factors      ScaleFactorDeltaBits == 6: CalculateOptimalDeltaLength :609-649, CriHcaPacking.WriteScaleFactors :262-295
  mixed_header_widths    raw and delta-coded channel headers side by side in the frames of one stream
  band_drops             CalculateNoiseLevel's retry loop :466-482 (a frame that does not fit at noise level 255)
  repeated_band_drops    ... run twice or more in one frame
  intensity_13           EncodeIntensityStereo's index runs into its bound :741-755
  intensity_0            ... a primary sub-frame without energy in either channel
  hfr_inverse            CalculateHfrScale scales a group by 1 / average, not by sqrt(2) :824-827
  hfr_zero               ... a group whose low bands average 0
  boundary_exit_equal    BinarySearchBoundary ends at low == high :544-547
  boundary_exit_probe    ... or at the final probe of `high` :549-551
  too_low                the retry loop runs out of bands: InvalidDataException("Bitrate is set too low.") :469-472 (ERROR_CASES)

Error returns.  -3 ("Bitrate is set too low.") is easy to reach: tests/host/analysis/hca_error_search.py crosses the lowest
bitrates CriHcaEncoder.Initialize accepts (1 bit/s upwards, 8000 / 44100 / 48000 Hz) with silence, full-scale noise, impulse
trains of period 4 and 64 and alternating full scale for 1-8 channels: of its 10920 encodes 8696 are refused, silence up to
9000 bit/s (eight channels: the empty headers alone do not fit) and every other signal up to 15500 bit/s (five channels).
ERROR_CASES holds four such streams.  -4 (the NotImplementedException of CalculateEvaluationBoundary :499) was reached by
none of those encodes, and cannot be: BinarySearchBoundary returns -1 only at low == high == 127, `low`
starts at 0 and is only ever set to mid = (low + high) / 2 while high - low > 1, so low <= 126 when the loop ends.  No case
is invented for it.
"""
import collections

import numpy as np

PATHS = ("raw_scale_factors", "mixed_header_widths", "band_drops", "repeated_band_drops", "intensity_13", "intensity_0",
         "hfr_inverse", "hfr_zero", "boundary_exit_equal", "boundary_exit_probe", "too_low")

# name; make() -> int16 [channels, samples]; quality, sample rate, bitrate (0: from the quality), limit_bitrate,
# loop (None or (start, end)); the paths the case is there for; reach(c): a condition on po.hca_encode_paths()
Case = collections.namedtuple("Case", "name make quality rate bitrate limit loop paths reach")


# ---------------------------------------------------------------- generators (seeded; no state outside the call)
def impulse_train(nch, n, period):
    """x[t] = 32767 where t % period == 0, else 0: a flat spectrum whose scale factors jump from band to band"""
    t = np.arange(n)
    return np.tile(np.where(t % period == 0, 32767, 0).astype(np.int16), (nch, 1))


def alternating(nch, n):
    """32767, -32768, 32767, ...: all energy at the Nyquist frequency, next to nothing in the bands HFR copies from"""
    t = np.arange(n)
    return np.tile(np.where(t % 2 == 0, 32767, -32768).astype(np.int16), (nch, 1))


def noise(nch, n, seed, amplitude=32768):
    return np.random.default_rng(seed).integers(-amplitude, amplitude, (nch, n)).astype(np.int16)


def ordinary(nch, n, first_channel=0):
    """the bench's synthetic channels (oracle/synth_oracle.c): what the older tests feed the encoder"""
    from oracle import pyoracle as po
    return po.synth_generate(nch, n, first_channel=first_channel)


def _with(x, edit):
    edit(x)
    return x


def _mixed(nch, n, rows):
    x = ordinary(nch, n)
    x[rows] = impulse_train(len(rows), n, 4)
    return x


def _left_silent(n, seed):
    return _with(noise(2, n, seed), lambda x: x[0].fill(0))


def _left_quiet(n, seed):
    return _with(noise(2, n, seed), lambda x: x.__setitem__(0, np.random.default_rng(seed + 1).integers(-40, 41, n)))


def _left_silent_right_silent_in_frames(n, seed, first, last):
    """left silent throughout; right full-scale noise, silent in samples [first, last): those sub-frames have no energy"""
    return _with(_left_silent(n, seed), lambda x: x[1, first:last].fill(0))


def _silent_then_noise(nch, n, seed, start):
    return _with(noise(nch, n, seed), lambda x: x[:, :start].fill(0))


# ---------------------------------------------------------------- reach conditions
def _delta_headers(c):
    return sum(c["sf_delta_bits"][1:6])


def _sub_frames(c):
    return sum(c["intensity"])


def _hfr_groups(c):
    return c["hfr_zero"] + c["hfr_sqrt2"] + c["hfr_inverse"]


def _half(count, of):
    return of > 0 and 2 * count >= of


REACH = {
    "raw_scale_factors": lambda c: _half(c["sf_delta_bits"][6], c["frames"]),
    "mixed_header_widths": lambda c: _half(c["sf_delta_bits"][6], c["frames"]) and _half(_delta_headers(c), c["frames"]),
    "band_drops": lambda c: _half(c["frames_with_band_drops"], c["frames"]),
    "repeated_band_drops": lambda c: c["frames_with_repeated_band_drops"] >= 1 and c["band_drops_frame_max"] >= 2,
    "intensity_13": lambda c: _half(c["intensity"][13], _sub_frames(c)),
    "intensity_0": lambda c: _half(c["intensity"][0], _sub_frames(c)),
    "hfr_inverse": lambda c: _half(c["hfr_inverse"], _hfr_groups(c)),
    "hfr_zero": lambda c: _half(c["hfr_zero"], _hfr_groups(c)),
    "boundary_exit_equal": lambda c: _half(c["boundary_exit_equal"], c["frames"]),
    "boundary_exit_probe": lambda c: _half(c["boundary_exit_probe"], c["frames"]),
    "too_low": lambda c: _half(c["error_minus3"], c["frames"]),
}


def _case(name, make, paths, quality="High", rate=48000, bitrate=0, limit=False, loop=None, also=None):
    def reach(c):
        return all(REACH[p](c) for p in paths) and (also is None or bool(also(c)))
    return Case(name, make, quality, rate, bitrate, limit, loop, tuple(paths), reach)


N = 10000            # 10 frames; the odd lengths below give 9-12

CASES = [
    # ---- scale factors written raw
    _case("raw_impulse4_mono_highest", lambda: impulse_train(1, N, 4), ["raw_scale_factors", "boundary_exit_equal"], "Highest"),
    _case("raw_impulse64_mono_highest", lambda: impulse_train(1, 11059, 64), ["raw_scale_factors"], "Highest"),
    _case("raw_impulse4_mono_highest_looping", lambda: impulse_train(1, N, 4), ["raw_scale_factors"], "Highest", loop=(1500, 9000)),
    # six discrete channels, the odd ones impulse trains: raw and delta-coded headers alternate inside every frame
    _case("raw_odd_channels_of_6_highest", lambda: _mixed(6, 9301, [1, 3, 5]), ["raw_scale_factors", "mixed_header_widths"], "Highest"),
    # the same inside the one-wave kernel's reach: two discrete channels (Highest has no stereo bands), the second an impulse train
    _case("raw_second_channel_of_2_highest", lambda: _mixed(2, 10700, [1]), ["raw_scale_factors", "mixed_header_widths"], "Highest"),
    # two stereo pairs (64-band secondaries with their 32 intensity bits), the second pair impulse trains
    _case("raw_second_pair_of_4_middle", lambda: _mixed(4, N, [2, 3]), ["raw_scale_factors", "mixed_header_widths"], "Middle"),
    # 44100 Hz at 100 kbit/s: 109 base bands and 7 HFR groups; raw headers, up to five drops a frame, 1 / average
    _case("raw_drops_hfr_impulse4_mono_44100", lambda: impulse_train(1, N, 4),
          ["raw_scale_factors", "band_drops", "repeated_band_drops", "hfr_inverse", "boundary_exit_probe"], rate=44100, bitrate=100000),
    # ---- bands dropped, the level searched again
    _case("drops_impulse4_mono_high", lambda: impulse_train(1, N, 4), ["band_drops", "repeated_band_drops"], "High"),
    _case("drops_noise_stereo_lowest_12000", lambda: noise(2, N, 1), ["band_drops", "repeated_band_drops"], "Lowest", bitrate=12000),
    _case("drops_noise_stereo_high_20000", lambda: noise(2, 12001, 2), ["band_drops"], "High", bitrate=20000),
    _case("drops_noise_3ch_lowest_24000", lambda: noise(3, N, 7), ["band_drops", "repeated_band_drops"], "Lowest", bitrate=24000),
    _case("drops_noise_6ch_lowest_48000", lambda: noise(6, 9500, 7), ["band_drops", "repeated_band_drops"], "Lowest", bitrate=48000),
    # ---- the intensity index at its bound, and at 0
    _case("intensity13_left_silent_lowest", lambda: _left_silent(N, 3), ["intensity_13", "hfr_zero"], "Lowest"),
    _case("intensity13_left_quiet_low", lambda: _left_quiet(N, 4), ["intensity_13"], "Low"),
    _case("intensity_0_and_13_stereo_lowest", lambda: _left_silent_right_silent_in_frames(N, 6, 0, 5120), ["intensity_0", "intensity_13"],
          "Lowest"),
    # two pairs: the first left silent / right noise (13), the second silent (0)
    _case("intensity_0_and_13_pairs_of_4_lowest", lambda: _with(noise(4, N, 10), lambda x: (x[0].fill(0), x[2:4].fill(0))),
          ["intensity_0", "intensity_13", "hfr_zero"], "Lowest"),
    # ---- the HFR group scale by the inverse
    _case("hfr_inverse_alternating_stereo_low", lambda: alternating(2, N), ["hfr_inverse", "boundary_exit_probe"], "Low"),
    _case("hfr_inverse_alternating_3ch_44100_90000", lambda: alternating(3, 10333), ["hfr_inverse", "band_drops", "boundary_exit_equal"],
          rate=44100, bitrate=90000),
]

# streams the reference refuses with InvalidDataException("Bitrate is set too low."): the oracle returns -3
ERROR_CASES = [
    _case("too_low_noise_mono_3000", lambda: noise(1, 5000, 21), ["too_low"], bitrate=3000, also=lambda c: c["band_drops"] > 0),
    _case("too_low_noise_5ch_15500", lambda: noise(5, 5000, 22), ["too_low"], bitrate=15500, also=lambda c: c["band_drops"] > 0),
    # silent frames fit, the later ones do not: the error comes from the middle of the stream
    _case("too_low_after_silent_frames_stereo_8000", lambda: _silent_then_noise(2, 8000, 23, 3000), ["too_low"], bitrate=8000,
          also=lambda c: c["frames"] - c["error_minus3"] >= 2 and c["band_drops_frame_max"] >= 2),
    # three channels at a bitrate that the ordinary channels still fit: the refused stream has neighbours that encode
    _case("too_low_impulse4_3ch_11250", lambda: impulse_train(3, 6000, 4), ["too_low"], bitrate=11250,
          also=lambda c: c["band_drops_frame_max"] >= 2),
]


def oracle_params(case, x):
    from oracle import pyoracle as po
    kw = dict(looping=True, loop_start=case.loop[0], loop_end=case.loop[1]) if case.loop else {}
    return po.hca_params(x.shape[0], x.shape[1], sample_rate=case.rate, quality=case.quality, bitrate=case.bitrate,
                         limit_bitrate=case.limit, **kw)


def oracle_encode(case):
    """-> (pcm, rc, HcaInfo, frames, path counters) of the oracle for the case"""
    from oracle import pyoracle as po
    x = case.make()
    rc, info, frames = po.hca_encode(x, oracle_params(case, x))
    return x, rc, info, frames, po.hca_encode_paths()


# what the oracle's counters (po.hca_encode_paths()) report for every case: test_hca_encoder_paths_host.py holds the oracle to
# this table, so a changed generator, parameter or counter shows up here first.  sf: channel headers by delta width 0..6 (6 = raw);
# intensity: primary sub-frames by index 0..13; hfr: groups (average 0, sqrt(2), 1 / average); drops: (iterations, most in a
# frame, frames with drops, frames with two or more); exits: boundary search (level 0: no search, low == high, final probe);
# hit_255: frames whose level search ended at 255; refused: frames that ended in "Bitrate is set too low."
RECORDED = {
    "raw_impulse4_mono_highest": dict(
        frames=10, sf=[0, 0, 0, 0, 2, 0, 8], intensity=[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
        hfr=(0, 0, 0), drops=(0, 0, 0, 0), exits=(0, 10, 0), hit_255=0, refused=0),
    "raw_impulse64_mono_highest": dict(
        frames=11, sf=[0, 0, 0, 0, 2, 0, 9], intensity=[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
        hfr=(0, 0, 0), drops=(0, 0, 0, 0), exits=(0, 10, 1), hit_255=0, refused=0),
    "raw_impulse4_mono_highest_looping": dict(
        frames=11, sf=[1, 0, 1, 0, 1, 0, 8], intensity=[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
        hfr=(0, 0, 0), drops=(0, 0, 0, 0), exits=(1, 8, 2), hit_255=0, refused=0),
    "raw_odd_channels_of_6_highest": dict(
        frames=10, sf=[0, 0, 2, 31, 3, 0, 24], intensity=[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
        hfr=(0, 0, 0), drops=(0, 0, 0, 0), exits=(0, 4, 6), hit_255=0, refused=0),
    "raw_second_channel_of_2_highest": dict(
        frames=11, sf=[0, 0, 2, 10, 1, 0, 9], intensity=[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
        hfr=(0, 0, 0), drops=(0, 0, 0, 0), exits=(0, 4, 7), hit_255=0, refused=0),
    "raw_second_pair_of_4_middle": dict(
        frames=10, sf=[0, 0, 2, 17, 5, 0, 16], intensity=[0, 0, 0, 2, 0, 0, 6, 130, 21, 1, 0, 0, 0, 0],
        hfr=(0, 0, 0), drops=(0, 0, 0, 0), exits=(0, 4, 6), hit_255=0, refused=0),
    "raw_drops_hfr_impulse4_mono_44100": dict(
        frames=10, sf=[0, 0, 0, 0, 2, 0, 8], intensity=[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
        hfr=(0, 14, 56), drops=(40, 5, 8, 8), exits=(0, 0, 10), hit_255=8, refused=0),
    "drops_impulse4_mono_high": dict(
        frames=10, sf=[0, 0, 8, 0, 2, 0, 0], intensity=[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
        hfr=(0, 0, 0), drops=(32, 4, 8, 8), exits=(0, 8, 2), hit_255=8, refused=0),
    "drops_noise_stereo_lowest_12000": dict(
        frames=10, sf=[0, 17, 3, 0, 0, 0, 0], intensity=[0, 0, 0, 0, 0, 3, 26, 23, 21, 6, 1, 0, 0, 0],
        hfr=(0, 80, 0), drops=(30, 3, 10, 10), exits=(0, 3, 7), hit_255=10, refused=0),
    "drops_noise_stereo_high_20000": dict(
        frames=12, sf=[0, 1, 3, 20, 0, 0, 0], intensity=[1, 0, 0, 0, 0, 2, 20, 44, 26, 3, 0, 0, 0, 0],
        hfr=(0, 84, 0), drops=(14, 2, 11, 3), exits=(0, 8, 4), hit_255=11, refused=0),
    "drops_noise_3ch_lowest_24000": dict(
        frames=10, sf=[0, 2, 9, 18, 1, 0, 0], intensity=[0, 0, 0, 0, 0, 4, 13, 37, 20, 6, 0, 0, 0, 0],
        hfr=(0, 100, 0), drops=(20, 2, 10, 10), exits=(0, 3, 7), hit_255=10, refused=0),
    "drops_noise_6ch_lowest_48000": dict(
        frames=10, sf=[0, 0, 22, 36, 2, 0, 0], intensity=[8, 0, 0, 0, 0, 9, 36, 61, 33, 12, 0, 1, 0, 0],
        hfr=(0, 200, 0), drops=(18, 2, 10, 8), exits=(0, 4, 6), hit_255=10, refused=0),
    "intensity13_left_silent_lowest": dict(
        frames=10, sf=[0, 3, 5, 12, 0, 0, 0], intensity=[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 80],
        hfr=(40, 40, 0), drops=(0, 0, 0, 0), exits=(0, 4, 6), hit_255=0, refused=0),
    "intensity13_left_quiet_low": dict(
        frames=10, sf=[0, 0, 1, 19, 0, 0, 0], intensity=[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 80],
        hfr=(0, 80, 0), drops=(0, 0, 0, 0), exits=(0, 6, 4), hit_255=0, refused=0),
    "intensity_0_and_13_stereo_lowest": dict(
        frames=10, sf=[10, 1, 2, 7, 0, 0, 0], intensity=[40, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 40],
        hfr=(60, 20, 0), drops=(0, 0, 0, 0), exits=(5, 0, 5), hit_255=0, refused=0),
    "intensity_0_and_13_pairs_of_4_lowest": dict(
        frames=10, sf=[20, 3, 7, 10, 0, 0, 0], intensity=[80, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 80],
        hfr=(120, 40, 0), drops=(0, 0, 0, 0), exits=(0, 3, 7), hit_255=0, refused=0),
    "hfr_inverse_alternating_stereo_low": dict(
        frames=10, sf=[0, 10, 8, 0, 2, 0, 0], intensity=[0, 0, 0, 0, 0, 0, 0, 80, 0, 0, 0, 0, 0, 0],
        hfr=(0, 16, 64), drops=(0, 0, 0, 0), exits=(0, 1, 9), hit_255=0, refused=0),
    "hfr_inverse_alternating_3ch_44100_90000": dict(
        frames=11, sf=[0, 30, 0, 0, 3, 0, 0], intensity=[6, 0, 0, 0, 0, 0, 0, 82, 0, 0, 0, 0, 0, 0],
        hfr=(0, 32, 144), drops=(9, 1, 9, 0), exits=(0, 9, 2), hit_255=9, refused=0),
    "too_low_noise_mono_3000": dict(
        frames=6, sf=[0, 0, 0, 0, 0, 0, 0], intensity=[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
        hfr=(0, 18, 0), drops=(6, 1, 6, 0), exits=(0, 0, 0), hit_255=6, refused=6),
    "too_low_noise_5ch_15500": dict(
        frames=6, sf=[0, 0, 0, 0, 0, 0, 0], intensity=[14, 0, 0, 1, 3, 13, 18, 17, 20, 4, 4, 2, 0, 0],
        hfr=(0, 72, 0), drops=(6, 1, 6, 0), exits=(0, 0, 0), hit_255=6, refused=6),
    "too_low_after_silent_frames_stereo_8000": dict(
        frames=8, sf=[4, 0, 0, 0, 0, 0, 0], intensity=[23, 0, 0, 0, 4, 4, 9, 11, 10, 3, 0, 0, 0, 0],
        hfr=(18, 30, 0), drops=(12, 2, 6, 6), exits=(2, 0, 0), hit_255=6, refused=6),
    "too_low_impulse4_3ch_11250": dict(
        frames=6, sf=[0, 3, 0, 0, 0, 0, 0], intensity=[0, 0, 0, 0, 0, 0, 0, 48, 0, 0, 0, 0, 0, 0],
        hfr=(0, 16, 44), drops=(12, 2, 6, 6), exits=(0, 1, 0), hit_255=6, refused=5),
}


def recorded_view(c):
    """po.hca_encode_paths() in the shape of RECORDED"""
    return dict(frames=c["frames"], sf=c["sf_delta_bits"], intensity=c["intensity"], hfr=(c["hfr_zero"], c["hfr_sqrt2"], c["hfr_inverse"]),
                drops=(c["band_drops"], c["band_drops_frame_max"], c["frames_with_band_drops"], c["frames_with_repeated_band_drops"]),
                exits=(c["frames_level_zero"], c["boundary_exit_equal"], c["boundary_exit_probe"]), hit_255=c["frames_level_search_hit_255"],
                refused=c["error_minus3"])

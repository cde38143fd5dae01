"""CPU side of the HCA encoder's rare-path cases (tests/hca_encoder_path_cases.py): every case takes the path it is there for
(the oracle's counters say so), every path has two cases, and the two restatements of CriHcaEncoder.cs -- oracle/hca_oracle.c
and oracle/pyref/crihca.py, written independently of each other -- agree on every case byte for byte.  The GPU tests
(test_gpu_hca_encoder_paths.py) compare the kernels with the oracle on the same cases; this file is what keeps those cases
on their paths."""
import functools

import numpy as np
import pytest

import hca_encoder_path_cases as pc
from oracle import pyoracle as po
from oracle.pyref import crihca as rhca

ALL = pc.CASES + pc.ERROR_CASES
BY_NAME = {c.name: c for c in ALL}
NAMES = [c.name for c in pc.CASES]
ERROR_NAMES = [c.name for c in pc.ERROR_CASES]


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    x, rc, info, frames, counters = pc.oracle_encode(BY_NAME[name])
    x.setflags(write=False)
    if frames is not None:
        frames.setflags(write=False)
    return x, rc, info, frames, counters


def _pyref_params(case, x):
    kw = dict(looping=True, loop_start=case.loop[0], loop_end=case.loop[1]) if case.loop else {}
    return rhca.Params(x.shape[0], case.rate, x.shape[1], quality=case.quality, bitrate=case.bitrate, limit_bitrate=case.limit, **kw)


def test_the_table_is_well_formed():
    assert len(set(BY_NAME)) == len(ALL)
    for case in ALL:
        assert case.paths and set(case.paths) <= set(pc.PATHS), case.name
        x = case.make()
        assert x.dtype == np.int16 and 1 <= x.shape[0] <= 8, case.name
        assert np.array_equal(x, case.make()), (case.name, "the generator is not seeded")
        rc, info = po.hca_init(pc.oracle_params(case, x))
        assert rc == 0 and info.frame_count <= 12, (case.name, rc, info.frame_count)
    assert any(c.loop for c in pc.CASES) and any(c.rate != 48000 for c in pc.CASES)
    assert any(c.make().shape[0] >= 3 and "band_drops" in c.paths for c in pc.CASES)


def test_counters_count_what_the_frames_hold():
    """the counters against what can be read back from the frames: one EncodeFrame and nch channel headers per frame, the
    3-bit delta widths at the head of the first channel's header, eight intensities per stereo pair and frame"""
    for name in NAMES:
        x, rc, info, frames, c = oracle_of(name)
        nch = x.shape[0]
        assert c["frames"] == info.frame_count and sum(c["sf_delta_bits"]) == nch * info.frame_count, name
        first = np.bincount((frames[:, 4] >> 5).astype(np.int64), minlength=8)        # bits 32..34: channel 0's delta width
        assert all(first[k] <= c["sf_delta_bits"][k] for k in range(7)) and first[7] == 0, name
        if nch == 1:
            assert list(first[:7]) == c["sf_delta_bits"], name
        pairs = {1: 0, 2: 1, 3: 1, 4: 2 if info.channel_config == 0 else 1, 5: 2 if info.channel_config <= 2 else 1, 6: 2, 7: 2, 8: 3}[nch]
        assert sum(c["intensity"]) == (8 * pairs * info.frame_count if info.stereo_band_count > 0 else 0), name
        assert c["boundary_exit_equal"] + c["boundary_exit_probe"] + c["frames_level_zero"] == info.frame_count, name
        assert c["frames_level_zero"] == int(np.sum(((frames[:, 2].astype(int) << 1) | (frames[:, 3] >> 7)) == 0)), name
        assert c["frames_with_band_drops"] <= c["frames_level_search_hit_255"] <= info.frame_count, name
        assert c["frames_with_repeated_band_drops"] <= c["frames_with_band_drops"] <= c["band_drops"], name
        assert c["error_minus3"] == c["error_minus4"] == 0, name


@pytest.mark.parametrize("name", NAMES + ERROR_NAMES)
def test_case_reaches_its_path(name):
    """the guard of the GPU tests: the oracle's counters for the case meet its reach condition, path by path"""
    case = BY_NAME[name]
    x, rc, info, frames, c = oracle_of(name)
    assert rc == (-3 if name in ERROR_NAMES else 0), (name, rc)
    for p in case.paths:
        assert pc.REACH[p](c), (name, p, c)
    assert case.reach(c), (name, c)


@pytest.mark.parametrize("name", NAMES + ERROR_NAMES)
def test_counters_are_the_recorded_ones(name):
    """the case table lists what the oracle reports for each case (RECORDED): exactly that, and -4 never"""
    c = oracle_of(name)[4]
    assert pc.recorded_view(c) == pc.RECORDED[name], name
    assert c["error_minus4"] == 0
    assert set(pc.RECORDED) == set(BY_NAME)


def test_every_path_has_two_cases():
    claimed = {p: [c.name for c in ALL if p in c.paths] for p in pc.PATHS}
    for p, names in claimed.items():
        assert len(names) >= 2, (p, names)
    # what the paths add up to over the table: all of it zero, or next to zero, over the older tests' 1899 frames
    total = {k: 0 for k in ("raw", "i13", "inverse", "drops")}
    for name in NAMES:
        c = oracle_of(name)[4]
        total["raw"] += c["sf_delta_bits"][6]
        total["i13"] += c["intensity"][13]
        total["inverse"] += c["hfr_inverse"]
        total["drops"] += c["band_drops"]
    assert total["raw"] >= 50 and total["i13"] >= 200 and total["inverse"] >= 200 and total["drops"] >= 150, total


@pytest.mark.parametrize("name", NAMES)
def test_second_restatement_agrees_with_the_oracle(name):
    """oracle/pyref/crihca.py on the case: HcaInfo, every frame and the PCM decoded from the frames equal the oracle's"""
    case = BY_NAME[name]
    x, rc, info, frames, _ = oracle_of(name)
    hi, fr = rhca.encode(x.tolist(), _pyref_params(case, x))
    for k, v in info.as_dict().items():
        if hasattr(hi, k):
            assert int(getattr(hi, k)) == v, (name, k)
    assert len(fr) == info.frame_count
    for i, f in enumerate(fr):
        assert f == bytes(frames[i]), (name, "frame", i)
    rc, dec = po.hca_decode(info, frames)
    assert rc == 0
    assert np.array_equal(np.asarray(rhca.decode(hi, fr), np.int16).reshape(dec.shape), dec), name


@pytest.mark.parametrize("name", ERROR_NAMES)
def test_second_restatement_refuses_the_same_frame(name):
    """"Bitrate is set too low.": pyref raises at the frame the oracle leaves zero (it goes on and reports -3 at the end), and
    the frames before it are the same"""
    case = BY_NAME[name]
    x, rc, info, frames, c = oracle_of(name)
    assert rc == -3
    refused = [i for i in range(info.frame_count) if not frames[i].any()]
    assert len(refused) == c["error_minus3"] > 0
    enc = rhca.Encoder(_pyref_params(case, x))
    got, block, i = [], [[0] * 1024 for _ in range(x.shape[0])], 0
    with pytest.raises(ValueError, match="Bitrate is set too low"):
        while len(got) < enc.hca.frame_count:                            # CriHcaFormat.cs:50-68, as rhca.encode feeds it
            k = min(x.shape[1] - i * 1024, 1024)
            for ch in range(x.shape[0]):
                if k > 0:
                    block[ch][0:k] = [int(v) for v in x[ch, 1024 * i:1024 * i + k]]
            got.extend(enc.encode(block))
            i += 1
    assert enc.frames_processed == refused[0], name
    for i, f in enumerate(got[:refused[0]]):
        assert f == bytes(frames[i]), (name, "frame", i)


def test_counters_leave_the_oracle_reentrant():
    """the counters are per thread and zeroed by every vgo_hca_encode: a second encode reports the same, and the batch driver's
    worker threads do not disturb the calling thread's"""
    x, rc, info, frames, c = oracle_of("drops_impulse4_mono_high")
    case = BY_NAME["drops_impulse4_mono_high"]
    p = pc.oracle_params(case, x)
    rc, _, again = po.hca_encode(x, p)
    mine = po.hca_encode_paths()
    assert rc == 0 and mine == c and np.array_equal(again, frames)
    rc, _, batch = po.hca_encode_batch(np.stack([x, x, x]), p, threads=3)
    assert rc == 0 and all(np.array_equal(b, frames.reshape(-1)) for b in batch)
    assert po.hca_encode_paths() == mine

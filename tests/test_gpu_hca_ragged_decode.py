"""vga_hca_decode_batch_v: streams of different lengths share one set of launches per length bucket (capi_hca.hip,
hca_decode_v_job; hca_decode_kernels.hip, RAGGED).  Every stream of every call must be what the oracle's decoder makes of its
frames alone (CriHcaDecoder.cs:11-192), bit for bit, and what one vga_hca_decode_batch call for it returns; the call's own
counters (vga_testing_hca_decode_v_stats) must show that the streams really shared their launches."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import test_gpu_host_paths as hp
from oracle import pyoracle as po
from vgaudio_amd import _lib, crihca

pytestmark = pytest.mark.gpu

i16p, u8p = _lib.i16p, _lib.u8p
SENTINEL = 0x7777
QUALITY = dict(Highest=1, High=2, Middle=3, Low=4, Lowest=5)


def L():
    return _lib.lib()


def _ptrs(t, arrays):
    return (t * len(arrays))(*[a.ctypes.data_as(t) if a is not None else None for a in arrays])


def shape(nch, n, quality="High", rate=48000, loop=None):
    return dict(nch=nch, n=n, quality=quality, rate=rate, loop=loop)


def encode(shapes, first_channel=0):
    """vga_hca_encode_batch_v of synthetic PCM -> [(HcaInfoC, frames as flat uint8)]"""
    ns = len(shapes)
    cps = (_lib.HcaParamsC * ns)()
    rows = []
    for s, sh in enumerate(shapes):
        cps[s] = _lib.HcaParamsC(QUALITY[sh["quality"]], 0, 0, sh["nch"], sh["rate"], sh["n"], 0, 0, 0)
        if sh["loop"]:
            cps[s].looping, cps[s].loop_start, cps[s].loop_end = 1, sh["loop"][0], sh["loop"][1]
        pcm = po.synth_generate(sh["nch"], sh["n"], first_channel=first_channel + 8 * s)
        rows += [np.ascontiguousarray(pcm[c]) if sh["n"] else None for c in range(sh["nch"])]
    infos = (_lib.HcaInfoC * ns)()
    for s in range(ns):
        _lib.check(L().vga_hca_encoder_initialize(C.byref(cps[s]), C.byref(infos[s])))
    outs = [np.zeros(infos[s].frame_count * infos[s].frame_size, np.uint8) for s in range(ns)]
    _lib.check(L().vga_hca_encode_batch_v(_ptrs(i16p, rows), ns, cps, infos, _ptrs(u8p, outs)))
    return [(_lib.HcaInfoC.from_buffer_copy(infos[s]), outs[s]) for s in range(ns)]


def oracle(info, frames):
    oi = po.HcaInfo()
    for f, _ in _lib.HcaInfoC._fields_:
        setattr(oi, f, getattr(info, f))
    rc, pcm = po.hca_decode(oi, frames.reshape(info.frame_count, info.frame_size))
    assert rc == 0
    return [pcm[c] for c in range(info.channel_count)]


def decode_v(streams, slack=9):
    """the raw call on arrays longer than needed and full of SENTINEL -> (status, [[channel arrays] per stream])"""
    ns = len(streams)
    infos = (_lib.HcaInfoC * ns)(*[h for h, _ in streams])
    outs = [[np.full(max(h.sample_count, 0) + slack, SENTINEL, np.int16) if h.sample_count > 0 else None
             for _ in range(h.channel_count)] for h, _ in streams]
    frames = [f if f is not None and f.size else None for _, f in streams]
    rc = L().vga_hca_decode_batch_v(infos, _ptrs(u8p, frames), ns, _ptrs(i16p, [r for o in outs for r in o]))
    return rc, outs


def stats():
    out = (C.c_longlong * 5)()
    assert L().vga_testing_hca_decode_v_stats(out, 5) == 5
    return dict(zip(("jobs", "chunks", "classes", "own", "slots"), out))


def assert_streams(got, want, what):
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (what, s)
        for c, (a, b) in enumerate(zip(g, w)):
            n = len(b)
            if a is None:
                assert n == 0, (what, s, c)
                continue
            assert np.array_equal(a[:n], b), (what, "stream", s, "channel", c, "samples", n)
            assert np.all(a[n:] == SENTINEL), (what, "wrote behind the stream's own samples", s, c)


def distinct_log_uniform(rng, count, lo, hi):
    seen = []
    while len(seen) < count:
        n = int(np.exp(rng.uniform(np.log(lo), np.log(hi))))
        if n not in seen:
            seen.append(n)
    return seen


# ---------------------------------------------------------------- 1 + 2. the main case and its counters
@pytest.fixture(scope="module")
def main_case():
    rng = np.random.default_rng(2026)
    lo, hi = 40 * 1024 - 128, 160 * 1024 - 128                       # 40 .. 160 frames (a plain stream leads in with 128 samples)
    shapes = [shape(1, n) for n in distinct_log_uniform(rng, 96, lo, hi)]
    shapes += [shape(2, n) for n in distinct_log_uniform(rng, 24, lo, hi)]
    shapes += [shape(6, 50_000)] * 4
    order = rng.permutation(len(shapes))                              # the three kinds interleaved
    shapes = [shapes[i] for i in order]
    assert {sh["nch"] for sh in shapes[:60]} == {1, 2, 6}
    streams = encode(shapes, first_channel=100)
    assert all(40 <= h.frame_count <= 160 for h, _ in streams if h.channel_count < 6)
    want = [oracle(h, f) for h, f in streams]
    return streams, want


def test_mixed_lengths_and_channel_counts_in_one_call_match_the_oracle(main_case):
    streams, want = main_case
    got = crihca.decode_streams([(crihca.HcaInfo(h), f) for h, f in streams])       # the Python mirror
    st = stats()
    for s, (g, w) in enumerate(zip(got, want)):
        for c in range(len(w)):
            assert np.array_equal(g[c], w[c]), (s, c)
    rc, raw = decode_v(streams)
    assert rc == _lib.VGA_OK
    assert_streams(raw, want, "raw call")
    # 2. the counters of that call: conditions, not measurements
    print("\n[hca ragged decode] stats of the main case:", st)
    assert st["jobs"] == 3                                            # one per channel count present
    assert st["classes"] == 3
    assert st["own"] == sum(h.frame_count for h, _ in streams)
    assert st["chunks"] <= 16 + 8 + 1
    assert st["slots"] <= 1.35 * st["own"], st


def test_every_stream_alone_through_the_equal_length_call_gives_the_same_bytes(main_case):
    streams, want = main_case
    for s, (h, f) in enumerate(streams):
        outs = [np.zeros(h.sample_count, np.int16) for _ in range(h.channel_count)]
        _lib.check(L().vga_hca_decode_batch(C.byref(h), _ptrs(u8p, [f]), 1, _ptrs(i16p, outs)))
        for c in range(h.channel_count):
            assert np.array_equal(outs[c], want[s][c]), (s, c)


# ---------------------------------------------------------------- 3. edge shapes among ordinary streams
def test_edge_shapes_in_one_call_with_ordinary_streams():
    shapes = [shape(1, 9000), shape(2, 20_000), shape(1, 0), shape(1, 700), shape(2, 896),
              shape(2, 21_000, loop=(3000, 17_000)), shape(2, 21_000), shape(1, 5555), shape(1, 5555), shape(2, 30_000)]
    streams = encode(shapes, first_channel=300)
    assert streams[2][0].sample_count == 0 and streams[3][0].frame_count == 1 and streams[4][0].frame_count == 1
    assert streams[5][0].inserted_samples != streams[6][0].inserted_samples
    # a stream of no frames at all: NULL frames, NULL rows
    empty = _lib.HcaInfoC.from_buffer_copy(streams[0][0])
    empty.sample_count = empty.frame_count = 0
    streams.insert(4, (empty, None))
    want = [oracle(h, f) if h.frame_count and h.sample_count else [np.zeros(0, np.int16)] * h.channel_count for h, f in streams]
    rc, got = decode_v(streams)
    assert rc == _lib.VGA_OK, L().vga_last_error()
    assert_streams(got, want, "edge shapes")
    assert not np.array_equal(got[8][0][:5555], got[9][0][:5555])    # the two streams of one shape hold different audio


# ---------------------------------------------------------------- 4. idle lanes must not flag
def test_a_short_stream_beside_a_long_one_in_one_chunk_is_not_a_bad_frame():
    """Lowest quality, mono: frames of 170 bytes, so streams of 1 to 7 frames lie within plan_buckets' additive slack of one
    another and share a chunk.  The scan's slots behind the short streams' own frames see zero-padding -- a zero sync word."""
    shapes = [shape(1, n, quality="Lowest") for n in (500, 7 * 1024 - 200, 2000, 6100, 800, 7 * 1024 - 300)]
    streams = encode(shapes, first_channel=500)
    assert [h.frame_count for h, _ in streams] == [1, 7, 3, 7, 1, 7]
    want = [oracle(h, f) for h, f in streams]
    with hp.hooks(pipeline=(0, 0, 64, 0)):
        rc, got = decode_v(streams)
        st = stats()
    assert rc == _lib.VGA_OK, L().vga_last_error()
    assert_streams(got, want, "one chunk")
    assert st["chunks"] == 1 and st["slots"] == 6 * 7 and st["own"] == 26, st
    # one byte of one stream's OWN sync word damaged: the call fails as one call for that stream does
    h, f = streams[2]
    bad = f.copy()
    bad[h.frame_size] ^= 0x40                                         # the second frame's first byte
    damaged = streams[:2] + [(h, bad)] + streams[3:]
    with hp.hooks(pipeline=(0, 0, 64, 0)):
        rc, _ = decode_v(damaged)
    assert rc == _lib.VGA_ERR_INVALID_DATA
    assert L().vga_last_error().decode() == "Invalid frame header"
    outs = [np.zeros(h.sample_count, np.int16)]
    assert L().vga_hca_decode_batch(C.byref(h), _ptrs(u8p, [bad]), 1, _ptrs(i16p, outs)) == _lib.VGA_ERR_INVALID_DATA


# ---------------------------------------------------------------- 5. invariance
@contextlib.contextmanager
def frames_per_group(n):
    old = L().vga_testing_hca_frames_per_group_this_thread(n)
    try:
        yield
    finally:
        L().vga_testing_hca_frames_per_group_this_thread(old)


@contextlib.contextmanager
def buckets_order(order):
    L().vga_testing_buckets_order_this_thread(order)
    try:
        yield
    finally:
        L().vga_testing_buckets_order_this_thread(0)


def test_pcm_does_not_depend_on_run_length_pipeline_shape_or_bucket_order(main_case):
    streams, want = main_case
    streams, want = streams[::3], want[::3]                          # 42 streams of the three kinds
    for n in (1, 3, 16):
        with frames_per_group(n):
            rc, got = decode_v(streams)
        assert rc == _lib.VGA_OK
        assert_streams(got, want, ("frames per group", n))
    for name, kw in hp.SHAPES.items():
        with hp.hooks(**kw):
            rc, got = decode_v(streams)
            assert stats()["chunks"] >= len(streams) // hp.CHUNK
        assert rc == _lib.VGA_OK
        assert_streams(got, want, ("pipeline", name))
    for order in (1, 2):
        with buckets_order(order):
            rc, got = decode_v(streams)
        assert rc == _lib.VGA_OK
        assert_streams(got, want, ("buckets order", order))


# ---------------------------------------------------------------- 6. dirty memory
@pytest.mark.parametrize("byte", [0xA5, 0xFF])
def test_the_main_case_on_poisoned_allocations(main_case, byte):
    """the slack behind the frames, the dimension table, the record slots nobody wrote and the PCM no frame covers: none of
    them may be read as data (include/vgaudio_hip_testing.h, vga_testing_poison_allocations)"""
    streams, want = main_case
    rc, clean = decode_v(streams)
    assert rc == _lib.VGA_OK
    assert L().vga_testing_poison_allocations(byte) == -1
    try:
        rc, got = decode_v(streams)
    finally:
        L().vga_testing_poison_allocations(-1)
    assert rc == _lib.VGA_OK
    for g, c in zip(got, clean):
        for a, b in zip(g, c):
            assert np.array_equal(a, b)
    assert_streams(got, want, ("poison", byte))


# ---------------------------------------------------------------- 7. seeded random sweep
@pytest.mark.parametrize("seed", range(6))
def test_random_streams_match_the_oracle(seed):
    rng = np.random.default_rng(77_000 + seed)
    qualities = [("High", "Low"), ("Highest", "Middle"), ("Middle", "Lowest")][seed % 3]
    rates = [(48000, 44100), (32000, 48000)][seed % 2]
    shapes = []
    for _ in range(int(rng.integers(20, 61))):
        n = int(np.exp(rng.uniform(0.0, np.log(200_000)))) if rng.random() < 0.5 else int(rng.integers(1, 200_001))
        shapes.append(shape(int(rng.integers(1, 3)), max(1, n), quality=str(rng.choice(qualities)), rate=int(rng.choice(rates))))
    streams = encode(shapes, first_channel=1000 * seed)
    want = [oracle(h, f) for h, f in streams]
    rc, got = decode_v(streams)
    assert rc == _lib.VGA_OK, L().vga_last_error()
    assert_streams(got, want, ("seed", seed))
    st = stats()
    assert st["jobs"] == len({h.channel_count for h, _ in streams}) and st["own"] == sum(h.frame_count for h, _ in streams)

"""Device-resident ragged ADX batches (include/vgaudio_hip/adx_ragged.h): vga_adx_encode_device_v / vga_adx_decode_device_v on
packed PCM rows and packed ADX rows.  Every channel must be what the oracle makes of it alone and what its own
vga_adx_*_device call makes of it, bit for bit; nothing outside a channel's own rows may change.  All buffers are larger than
needed and full of junk.  The header is outside the lists the older test files enumerate, so this file carries its own table
(CASES) of which test exercises which function; tests/test_adx_ragged_device_host.py holds that table to the header."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from test_gpu_device_streams import delay  # noqa: F401  (the calibrated GPU delay that makes a caller's stream busy)
from vgaudio_amd import _lib
from vgaudio_amd.criadx import RaggedAdx

pytestmark = pytest.mark.gpu

# function of the header -> the tests below that call it
CASES = {
    "vga_adx_ragged_layout_for": ["test_layout_of_the_object_is_the_host_layout"],
    "vga_adx_ragged_create": ["test_encode_and_decode_match_oracle", "test_stats"],
    "vga_adx_ragged_destroy": ["test_encode_and_decode_match_oracle"],
    "vga_adx_ragged_channels": ["test_layout_of_the_object_is_the_host_layout"],
    "vga_adx_ragged_totals_of": ["test_layout_of_the_object_is_the_host_layout"],
    "vga_adx_ragged_offsets": ["test_layout_of_the_object_is_the_host_layout"],
    "vga_adx_encode_device_v": ["test_encode_and_decode_match_oracle", "test_channel_counts_around_a_group", "test_own_calls_agree",
                                "test_general_path_for_other_frame_sizes_and_padded_streams", "test_uniform_object",
                                "test_uniform_object_with_seams", "test_bytes_do_not_depend_on_poison", "test_round_trip_on_a_busy_stream_and_two_streams_at_once",
                                "test_zero_length_channel_under_v4_without_padding", "test_refused_layouts_launch_nothing"],
    "vga_adx_decode_device_v": ["test_encode_and_decode_match_oracle", "test_channel_counts_around_a_group", "test_own_calls_agree",
                                "test_general_path_for_other_frame_sizes_and_padded_streams", "test_uniform_object_with_seams",
                                "test_bytes_do_not_depend_on_poison", "test_round_trip_on_a_busy_stream_and_two_streams_at_once",
                                "test_bad_filter_index_marks_its_channel_only", "test_zero_length_channel_under_v4_without_padding",
                                "test_refused_layouts_launch_nothing"],
}

SENTINEL = 0x7777
JUNK = 0xEE
EXTRA = 64
LONGEST = 40000                                                        # 1250 frames
SQUARE, SILENT = 5, 9                                                  # channels that carry the square wave / digital silence

PARAM_SETS = {
    "default": {},
    "version3": {"version": 3},
    "exponential": {"type": 4},
    "fixed1": {"type": 2, "filter": 1},
    "fixed3": {"type": 2, "filter": 3},
    "rate22050": {"sample_rate": 22050},
    "frame34": {"frame_size": 34},
    "padding10": {"padding": 10, "history": 1234},
    "padding40": {"padding": 40, "history": -321},
}


def torch():
    import torch as t
    return t


def L():
    return _lib.lib()


def up(a):
    return torch().from_numpy(np.ascontiguousarray(a)).cuda()


def cparams(name):
    return _lib.AdxParams.from_buffer_copy(po.adx_params(**PARAM_SETS[name]))


@contextlib.contextmanager
def hooks(segments=0, force_open=0):
    old_s = L().vga_testing_gc_encoder_segments_this_thread(segments)
    old_f = L().vga_testing_force_open_seams_this_thread(force_open)
    try:
        yield
    finally:
        torch().cuda.synchronize()
        L().vga_testing_force_open_seams_this_thread(old_f)
        L().vga_testing_gc_encoder_segments_this_thread(old_s)


def stats(r):
    v = (C.c_longlong * 10)()
    assert L().vga_testing_adx_ragged_stats(r._h, v, 10) == 10
    return list(v)


_signals = {}


def signals():
    """[150, LONGEST]: the synthetic set from channel 90 on (93, the slowest to fall into step, among them), one frame-periodic
    square whose seams never close, one all-zero channel"""
    if "pcm" not in _signals:
        pcm = po.synth_generate(150, LONGEST, first_channel=90)
        i = np.arange(LONGEST)
        pcm[SQUARE] = (12000 * np.sign(np.sin(2 * np.pi * i / 64))).astype(np.int16)
        pcm[SILENT] = 0
        _signals["pcm"] = pcm
    return _signals["pcm"]


def seam_lengths(segments):
    """three lengths around a piece boundary of the plan an object of these sizes gets: read from the hook of a probe object
    (the plan follows the longest channel)"""
    with hooks(segments):
        r = RaggedAdx(cparams("default"), [LONGEST])
        v = stats(r)
        r.close()
    out = []
    for seg in (v[3], v[6]):                                           # the encoder's pieces, the decoder's
        out += [min(seg * 32 + d, LONGEST) for d in (-1, 0, 1)]
    return out


def lengths_for(nch, segments=0):
    """caller order, not sorted: the edges of a frame, a pair, a group of eight frames and 64 frames; two equal lengths; the
    longest; lengths around a piece boundary; a seeded fill"""
    if nch == 1:
        return [LONGEST]
    core = [2049, 1, LONGEST, 30011, 31, 35000, 32, 33, 63, 64, 65, 255, 777, 256, 257, 2047, 2048, 2, 777]   # ([3]: channel 93; [5]: the square)
    rng = np.random.default_rng(1000 + nch)
    out = core + seam_lengths(segments) + [int(v) for v in rng.integers(1, LONGEST + 1, 150)]
    return out[:nch]


_oracle = {}


def oracle(name, c, n):
    """(ADX bytes, decoded PCM) of channel c's first n samples under the parameter set, computed once"""
    key = (name, c, n)
    if key not in _oracle:
        p = po.adx_params(**PARAM_SETS[name])
        adx = po.adx_encode(signals()[c, :n], p)
        p = po.adx_params(**PARAM_SETS[name])                          # (the encoder sets History)
        _oracle[key] = (adx, po.adx_decode(adx, n, p))
    return _oracle[key]


class Batch:
    """a ragged object over channels 0 .. len(lengths) - 1 of the signal set and junk-filled packed buffers on the device"""

    def __init__(self, name, lengths):
        self.name, self.lengths = name, list(lengths)
        self.p = cparams(name)
        self.r = RaggedAdx(self.p, self.lengths)
        self.t, self.po, self.ao = self.r.totals, self.r.pcm_offsets, self.r.adx_offsets
        self.want = [oracle(name, c, n) for c, n in enumerate(self.lengths)]

    def close(self):
        self.r.close()

    def pcm_image(self, fill=True):
        img = np.full(self.t.pcm_samples + EXTRA, SENTINEL, np.int16)
        if fill:
            for c, (n, at) in enumerate(zip(self.lengths, self.po)):
                img[at:at + n] = signals()[c, :n]
        return img

    def adx_image(self, fill=True):
        img = np.full(self.t.adx_bytes + EXTRA, JUNK, np.uint8)
        if fill:
            for (adx, _), at in zip(self.want, self.ao):
                img[at:at + adx.size] = adx
        return img

    def workspace(self, encode):
        n = self.t.encode_workspace_bytes if encode else self.t.decode_workspace_bytes
        return torch().full((n + EXTRA,), 0xCD, dtype=torch().uint8, device="cuda")

    def status(self):
        return torch().zeros(len(self.lengths) + 1, dtype=torch().int32, device="cuda")

    def encode(self, stream=None):
        pcm, adx = up(self.pcm_image()), up(self.adx_image(fill=False))
        hist = torch().full((len(self.lengths) + 1,), SENTINEL, dtype=torch().int16, device="cuda")
        self.r.encode_device(pcm, adx, self.workspace(True), hist, stream=stream)
        return pcm, adx, hist

    def decode(self, adx_img=None, stream=None):
        adx = up(self.adx_image() if adx_img is None else adx_img)
        pcm, st = up(self.pcm_image(fill=False)), self.status()
        self.r.decode_device(adx, pcm, self.workspace(False), st, stream=stream)
        return adx, pcm, st

    def history(self, c):
        """what vga_adx_encode_device reports for the channel (CriAdxCodec.cs:69-74)"""
        if self.p.version == 4 and self.p.padding == 0 and self.lengths[c] > 0:
            return int(signals()[c, 0])
        return int(self.p.history)

    def check_adx(self, got, what, hist=None):
        own = np.zeros(got.size, bool)
        for c, ((adx, _), at) in enumerate(zip(self.want, self.ao)):
            own[at:at + adx.size] = True
            assert np.array_equal(got[at:at + adx.size], adx), (what, "channel", c, "samples", self.lengths[c])
        assert np.all(got[~own] == JUNK), (what, "wrote outside the channels' own rows")
        if hist is not None:
            assert [int(v) for v in hist[:-1]] == [self.history(c) for c in range(len(self.lengths))], what
            assert int(hist[-1]) == SENTINEL

    def check_pcm(self, got, what, skip=()):
        own = np.zeros(got.size, bool)
        for c, ((_, pcm), at) in enumerate(zip(self.want, self.po)):
            own[at:at + pcm.size] = True
            if c not in skip:
                assert np.array_equal(got[at:at + pcm.size], pcm), (what, "channel", c, "samples", self.lengths[c])
        assert np.all(got[~own] == SENTINEL), (what, "wrote outside the channels' own rows")

    def round_trip(self, what, paths=None):
        pcm, adx, hist = self.encode()
        _, out, st = self.decode()
        torch().cuda.synchronize()
        self.check_adx(adx.cpu().numpy(), (what, "encode"), hist.cpu().numpy())
        assert np.array_equal(pcm.cpu().numpy(), self.pcm_image()), "d_pcm is an input"
        self.check_pcm(out.cpu().numpy(), (what, "decode"))
        assert np.all(st.cpu().numpy() == 0)
        if paths:
            enc, dec = C.c_int(), C.c_int()
            L().vga_testing_adx_last_path_this_thread(C.byref(enc), C.byref(dec))
            assert (enc.value, dec.value) == paths == tuple(stats(self.r)[8:10]), what


@contextlib.contextmanager
def batch_of(name, lengths):
    b = Batch(name, lengths)
    try:
        yield b
    finally:
        torch().cuda.synchronize()
        b.close()


# ---------------------------------------------------------------- encode and decode against the oracle
PLANS = [(0, 0), (12, 0), (12, 1), (12, 3), (40, 0), (40, 1), (40, 3), (0, 3)]


@pytest.mark.parametrize("name", ["default", "version3", "exponential", "fixed1", "fixed3", "rate22050"])
def test_encode_and_decode_match_oracle(name):
    """150 channels (the last group is partial) under every piece plan and seam mode; frame size 18 without padding must
    take the time-piece kernels"""
    for segments, force in (PLANS if name == "default" else [(0, 0), (12, 1), (40, 3)]):
        lengths = lengths_for(150, segments)
        assert lengths[SQUARE] > 30000 and lengths[3] > 30000 and len(set(lengths)) < len(lengths) and max(lengths) == LONGEST
        with hooks(segments):
            b = Batch(name, lengths)                                   # (the plan is made at create)
        try:
            v = stats(b.r)
            if segments == 12:
                assert (v[2], v[3]) == (12, 106)
            if segments == 40:
                assert (v[2], v[3], v[5], v[6]) == (19, 66, 40, 32)
            with hooks(0, force):                                      # (the seam mode is read at call time)
                b.round_trip((name, segments, force), paths=(1, 1))
        finally:
            torch().cuda.synchronize()
            b.close()


@pytest.mark.parametrize("nch", [1, 63, 64, 65])
def test_channel_counts_around_a_group(nch):
    for segments, force in ((12, 0), (40, 3)):
        with hooks(segments):
            b = Batch("default", lengths_for(nch, segments))
        try:
            assert stats(b.r)[1] == (nch + 63) // 64
            with hooks(0, force):
                b.round_trip((nch, segments, force), paths=(1, 1))
        finally:
            torch().cuda.synchronize()
            b.close()


def own_encode(p, pcm):
    t, n = torch(), len(pcm)
    nbytes = L().vga_adx_encoded_byte_count(n, C.byref(p))
    src = t.zeros(max((n + 7) // 8 * 8, 8), dtype=t.int16, device="cuda")
    src[:n] = up(pcm)
    out = t.full((max((nbytes + 15) // 16 * 16, 16),), JUNK, dtype=t.uint8, device="cuda")
    hist = t.zeros(1, dtype=t.int16, device="cuda")
    _lib.check(L().vga_adx_encode_device(src.data_ptr(), src.numel(), 1, n, C.byref(p), out.data_ptr(), out.numel(), hist.data_ptr(), None))
    t.cuda.synchronize()
    return out.cpu().numpy()[:nbytes], int(hist.item())


def own_decode(p, adx, n):
    t = torch()
    src = t.zeros((adx.size + 15) // 16 * 16 + 16, dtype=t.uint8, device="cuda")
    src[:adx.size] = up(adx)
    out = t.full((max((n + 7) // 8 * 8, 8),), SENTINEL, dtype=t.int16, device="cuda")
    st = t.zeros(1, dtype=t.int32, device="cuda")
    _lib.check(L().vga_adx_decode_device(src.data_ptr(), src.numel(), adx.size, 1, n, C.byref(p), out.data_ptr(), out.numel(), st.data_ptr(), None))
    t.cuda.synchronize()
    return out.cpu().numpy()[:n], int(st.item())


@pytest.mark.parametrize("name", ["default", "fixed1", "padding10"])
def test_own_calls_agree(name):
    """a handful of channels: the bytes of the packed call are those of one vga_adx_*_device call per channel, history included"""
    lengths = lengths_for(65, 12)
    with hooks(12):
        b = Batch(name, lengths)
    try:
        _, adx, hist = b.encode()
        _, pcm, _ = b.decode()
        torch().cuda.synchronize()
        adx, hist, pcm = adx.cpu().numpy(), hist.cpu().numpy(), pcm.cpu().numpy()
        for c in (0, 1, 2, SQUARE, SILENT, 12, 17, 40):
            n = lengths[c]
            got, h = own_encode(b.p, signals()[c, :n])
            assert np.array_equal(adx[b.ao[c]:b.ao[c] + got.size], got) and int(hist[c]) == h, (name, c)
            own, status = own_decode(b.p, got, n)
            assert status == 0 and np.array_equal(pcm[b.po[c]:b.po[c] + n], own), (name, c)
    finally:
        torch().cuda.synchronize()
        b.close()


@pytest.mark.parametrize("name", ["frame34", "padding10", "padding40"])
def test_general_path_for_other_frame_sizes_and_padded_streams(name):
    """the general lane-per-channel kernel on the same tables (the hook says 2): other frame sizes; padded streams with a start
    history, lengths whose padded decode leaves a zero tail (CriAdxCodec.cs:18-34) and a channel of no samples in the middle"""
    lengths = lengths_for(65, 0)
    if name != "frame34":                                              # (version 4 without padding: the reference reads pcm[0])
        lengths[30] = 0
    lengths[31], lengths[32] = 40, 23                                  # padding 10: the first frame yields 22 samples of 32
    with batch_of(name, lengths) as b:
        assert b.t.encode_workspace_bytes == b.t.decode_workspace_bytes == 0
        if name != "frame34":
            pad = PARAM_SETS[name]["padding"]
            short = [c for c, n in enumerate(lengths) if 0 < n and (n + 31) // 32 * 32 - pad % 32 < n]
            assert short, "no length leaves a zero tail"
            assert any(np.all(b.want[c][1][-1:] == 0) for c in short)
        b.round_trip(name, paths=(2, 2))


# ---------------------------------------------------------------- all lengths equal
def test_uniform_object():
    """the bytes equal ONE vga_adx_encode_device call on all channels at the rounded pitches"""
    t, n, nch = torch(), 5000, 70
    with batch_of("default", [n] * nch) as b:
        _, adx, hist = b.encode()
        t.cuda.synchronize()
        b.check_adx(adx.cpu().numpy(), "uniform", hist.cpu().numpy())
        pitch, nbytes = (n + 7) // 8 * 8, L().vga_adx_encoded_byte_count(n, C.byref(b.p))
        out_pitch = (nbytes + 15) // 16 * 16
        assert list(b.po) == [c * pitch for c in range(nch)] and list(b.ao) == [c * out_pitch for c in range(nch)]
        src = up(b.pcm_image())
        out = t.full((nch * out_pitch,), JUNK, dtype=t.uint8, device="cuda")
        h = t.zeros(nch, dtype=t.int16, device="cuda")
        _lib.check(L().vga_adx_encode_device(src.data_ptr(), pitch, nch, n, C.byref(b.p), out.data_ptr(), out_pitch, h.data_ptr(), None))
        t.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), adx.cpu().numpy()[:nch * out_pitch])
        assert np.array_equal(h.cpu().numpy(), hist.cpu().numpy()[:nch])


def test_uniform_object_with_seams():
    """70 channels of 24 589 samples -- 769 frames: twelve pieces under the hook (the encoder's at its 64-frame floor) and a
    partial last frame -- under seam modes 0, 1 and 3: the packed object and ONE vga_adx_encode_device / vga_adx_decode_device
    call on the same rounded pitches run their direct, fix-up, tail and REPAIR kernels on the same rows.  The kernels of the
    two calls are shells over the same bodies, so both must write the same ADX bytes, histories, PCM and status words, and the
    packed result is the oracle's"""
    t, n, nch = torch(), 24589, 70
    with hooks(12):
        b = Batch("default", [n] * nch)                                # (the plan is made at create)
    try:
        v = stats(b.r)
        assert (v[2], v[3], v[5], v[6]) == (12, 66, 12, 66)
        pitch, nbytes = (n + 7) // 8 * 8, L().vga_adx_encoded_byte_count(n, C.byref(b.p))
        out_pitch = (nbytes + 15) // 16 * 16
        assert list(b.po) == [c * pitch for c in range(nch)] and list(b.ao) == [c * out_pitch for c in range(nch)]
        for force in (0, 1, 3):
            with hooks(12, force):                                     # (the equal-length call plans when it is called)
                _, adx, hist = b.encode()
                _, pcm, st = b.decode()
                src = up(b.pcm_image())
                out = t.full((nch * out_pitch,), JUNK, dtype=t.uint8, device="cuda")
                h = t.zeros(nch, dtype=t.int16, device="cuda")
                _lib.check(L().vga_adx_encode_device(src.data_ptr(), pitch, nch, n, C.byref(b.p), out.data_ptr(), out_pitch,
                                                     h.data_ptr(), None))
                back = t.full((nch * pitch,), SENTINEL, dtype=t.int16, device="cuda")
                one = t.zeros(1, dtype=t.int32, device="cuda")
                _lib.check(L().vga_adx_decode_device(out.data_ptr(), out_pitch, nbytes, nch, n, C.byref(b.p), back.data_ptr(), pitch,
                                                     one.data_ptr(), None))
                t.cuda.synchronize()
            adx, hist, pcm, st = adx.cpu().numpy(), hist.cpu().numpy(), pcm.cpu().numpy(), st.cpu().numpy()
            assert np.array_equal(out.cpu().numpy(), adx[:nch * out_pitch]), force
            assert np.array_equal(h.cpu().numpy(), hist[:nch]), force
            assert np.array_equal(back.cpu().numpy(), pcm[:nch * pitch]), force
            assert np.all(st[:nch] == int(one.item())) and st[nch] == 0, force
            b.check_adx(adx, ("uniform", force), hist)
            b.check_pcm(pcm, ("uniform", force))
            assert np.all(st == 0), force
    finally:
        torch().cuda.synchronize()
        b.close()


# ---------------------------------------------------------------- poison mode
@pytest.mark.parametrize("mode", ["poison-a5", "poison-ff", "off"])
def test_bytes_do_not_depend_on_poison(mode):
    old = L().vga_testing_poison_allocations(int(mode[-2:], 16) if mode != "off" else -1)
    try:
        for name, segments, force in (("default", 12, 0), ("default", 40, 3), ("version3", 12, 1), ("padding10", 0, 0)):
            with hooks(segments):
                b = Batch(name, lengths_for(65, segments))             # (created under the mode: its tables are poisoned first)
            try:
                with hooks(0, force):
                    b.round_trip((mode, name, segments, force))
            finally:
                torch().cuda.synchronize()
                b.close()
    finally:
        torch().cuda.synchronize()
        L().vga_testing_poison_allocations(old if old >= 0 else -1)


# ---------------------------------------------------------------- a busy caller stream, two streams at once
POOL_STREAMS = 32                                                      # torch hands out this many streams, round robin


def two_streams():
    """Two streams for this file, taken so that the files that run after it find torch's stream pool as they would without
    it.  torch.cuda.Stream() walks a pool of 32 streams round robin, and a process has only a few hardware queues (four by
    default), so which two streams a later test gets -- and whether they can run side by side, which the two-calls-in-flight
    tests of test_gpu_device_streams.py and test_gpu_dirty_memory.py need of two neighbouring pool streams -- depends on
    how many streams were taken before it and on the order in which the pool's streams were first used.  This file takes
    one whole turn of the pool (the imported `delay` fixture has taken the first) and uses every stream once, in order:
    the round robin stands where it stood, and neighbouring pool streams were first used one after the other."""
    t = torch()
    taken = [t.cuda.Stream() for _ in range(POOL_STREAMS - 1)]
    for s in taken:
        with t.cuda.stream(s):
            t.zeros(1, device="cuda")
    t.cuda.synchronize()
    return taken[0], taken[1]


def test_round_trip_on_a_busy_stream_and_two_streams_at_once(delay):  # noqa: F811
    t = torch()
    cycles, ms = delay
    with hooks(12):
        b = Batch("default", lengths_for(65, 12))
    try:
        with hooks(0, 1):                                              # every seam open: fix-up, tail and their fills on the stream
            A, B = two_streams()
            out = {}
            for name, S, busy in (("warm", A, False), ("A", A, True), ("B", B, False)):
                with t.cuda.stream(S):
                    pcm_in, adx = up(b.pcm_image()), up(b.adx_image(fill=False))
                    pcm_out, st = up(b.pcm_image(fill=False)), b.status()
                    ws_e, ws_d = b.workspace(True), b.workspace(False)     # a workspace of its own per stream
                    if busy:
                        t.cuda._sleep(cycles)
                b.r.encode_device(pcm_in, adx, ws_e, None, stream=S)  # encode, then decode what it wrote: no host synchronisation
                b.r.decode_device(adx, pcm_out, ws_d, st, stream=S)
                if busy:
                    assert not S.query(), "the caller's stream was idle when the calls returned (they waited for it)"
                out[name] = (adx, pcm_out, st, pcm_in, ws_e, ws_d)
                if name == "warm":
                    S.synchronize()
            B.synchronize()
            A.synchronize()
            for name in ("A", "B"):
                adx, pcm_out, st = out[name][:3]
                assert np.all(st.cpu().numpy() == 0)
                b.check_adx(adx.cpu().numpy(), name)
                b.check_pcm(pcm_out.cpu().numpy(), name)
            assert t.equal(out["A"][0], out["B"][0]) and t.equal(out["A"][1], out["B"][1])
    finally:
        t.cuda.synchronize()
        b.close()


# ---------------------------------------------------------------- a bad frame marks its own channel
def test_bad_filter_index_marks_its_channel_only():
    lengths = lengths_for(65, 12)
    marked = (2, 40)                                                   # the longest channel and a seeded one
    with hooks(12):
        b = Batch("fixed1", lengths)
    try:
        img = b.adx_image()
        for c in marked:
            frames = b.want[c][0].size // 18
            assert frames >= 3
            at = b.ao[c] + (frames // 2) * 18
            img[at] = (img[at] & 0x1F) | (5 << 5)                      # the filter bits of a middle frame's header
        adx, pcm, st = b.decode(adx_img=img)                           # (the wrapper raises on a non-zero return value)
        torch().cuda.synchronize()
        status = st.cpu().numpy()
        assert all(status[c] == 1 for c in marked)
        assert np.all(np.delete(status, marked) == 0)
        b.check_pcm(pcm.cpu().numpy(), "bad filter", skip=marked)
        assert np.array_equal(adx.cpu().numpy(), img), "d_adx is an input"
    finally:
        torch().cuda.synchronize()
        b.close()


# ---------------------------------------------------------------- a channel of no samples where the reference reads pcm[0]
def test_zero_length_channel_under_v4_without_padding():
    lengths = lengths_for(20, 0)
    lengths[7] = lengths[11] = 0
    with batch_of("default", lengths) as b:
        pcm, adx = up(b.pcm_image()), up(b.adx_image(fill=False))
        with pytest.raises(_lib.ArgumentError, match="channel 7 "):
            b.r.encode_device(pcm, adx, b.workspace(True))
        torch().cuda.synchronize()
        assert np.all(adx.cpu().numpy() == JUNK)
        _, out, st = b.decode()                                        # the object is still good for decoding
        torch().cuda.synchronize()
        b.check_pcm(out.cpu().numpy(), "after the refusal")
        assert np.all(st.cpu().numpy() == 0)
    with batch_of("version3", lengths) as b:                           # version 3 encodes it: no bytes, the history is the parameter's
        b.round_trip("version 3 with empty channels", paths=(1, 1))


# ---------------------------------------------------------------- the object's numbers
def test_layout_of_the_object_is_the_host_layout():
    for name in ("default", "frame34", "padding40"):
        lengths = lengths_for(150, 0)
        po_, ao_, tot = RaggedAdx.layout(cparams(name), lengths)
        with batch_of(name, lengths) as b:
            assert b.r.channels == len(lengths) == L().vga_adx_ragged_channels(b.r._h)
            assert np.array_equal(po_, b.po) and np.array_equal(ao_, b.ao)
            assert all(getattr(tot, f) == getattr(b.t, f) for f, _ in tot._fields_)


def test_stats():
    for segments in (0, 12, 40):
        lengths = lengths_for(150, segments)
        with hooks(segments):
            r = RaggedAdx(cparams("default"), lengths)
        v = stats(r)
        r.close()
        frames = [(n + 31) // 32 for n in lengths]
        group_frames = sorted(frames, reverse=True)[::64]
        assert v[0] == sum(frames) and v[1] == len(group_frames) == 3
        assert v[2] <= 64 and v[5] <= 64
        assert v[4] == sum((gf + v[3] - 1) // v[3] for gf in group_frames)
        assert v[7] == sum((gf + v[6] - 1) // v[6] for gf in group_frames)
        assert v[2] * v[3] >= 1250 > (v[2] - 1) * v[3] and v[5] * v[6] >= 1250 > (v[5] - 1) * v[6]
        assert (v[8], v[9]) == (1, 1)


# ---------------------------------------------------------------- refused layouts
def test_refused_layouts_launch_nothing():
    t = torch()
    ARG = _lib.VGA_ERR_ARGUMENT
    with batch_of("default", lengths_for(65, 0)) as b:
        pcm_in, adx_out = up(b.pcm_image()), up(b.adx_image(fill=False))
        adx_in, pcm_out = up(b.adx_image()), up(b.pcm_image(fill=False))
        ws, st = b.workspace(True), b.status()
        hist = t.full((66,), SENTINEL, dtype=t.int16, device="cuda")
        h, need_e, need_d = b.r._h, b.t.encode_workspace_bytes, b.t.decode_workspace_bytes
        assert need_e >= need_d > 0
        enc, dec = L().vga_adx_encode_device_v, L().vga_adx_decode_device_v
        P, A, W, H, S = pcm_in.data_ptr(), adx_out.data_ptr(), ws.data_ptr(), hist.data_ptr(), st.data_ptr()
        assert enc(h, P + 2, A, H, W, need_e, None) == ARG
        assert enc(h, P, A + 2, H, W, need_e, None) == ARG
        assert enc(h, P, A, H, W, need_e - 16, None) == ARG
        assert enc(h, P, A, H, W + 8, need_e + 8, None) == ARG
        assert enc(None, P, A, H, W, need_e, None) == ARG
        assert enc(h, None, A, H, W, need_e, None) == ARG and enc(h, P, None, H, W, need_e, None) == ARG
        assert enc(h, P, A, H, None, need_e, None) == ARG
        P2, A2 = pcm_out.data_ptr(), adx_in.data_ptr()
        assert dec(h, A2 + 2, P2, W, need_d, S, None) == ARG
        assert dec(h, A2, P2 + 2, W, need_d, S, None) == ARG
        assert dec(h, A2, P2, W, need_d - 16, S, None) == ARG
        assert dec(h, A2, P2, W + 8, need_d + 8, S, None) == ARG
        assert dec(None, A2, P2, W, need_d, S, None) == ARG
        assert dec(h, None, P2, W, need_d, S, None) == ARG and dec(h, A2, None, W, need_d, S, None) == ARG
        assert dec(h, A2, P2, None, need_d, S, None) == ARG and dec(h, A2, P2, W, need_d, None, None) == ARG
        t.cuda.synchronize()
        assert np.all(pcm_out.cpu().numpy() == SENTINEL) and np.all(adx_out.cpu().numpy() == JUNK)
        assert np.all(ws.cpu().numpy() == 0xCD) and np.all(st.cpu().numpy() == 0) and np.all(hist.cpu().numpy() == SENTINEL)
        # exactly at the minimum: buffers of the totals' sizes, a workspace of exactly the bytes asked for
        pcm_min, adx_min = up(b.pcm_image()[:b.t.pcm_samples]), up(b.adx_image(fill=False)[:b.t.adx_bytes])
        ws_min = t.full((need_e,), 0xCD, dtype=t.uint8, device="cuda")
        assert enc(h, pcm_min.data_ptr(), adx_min.data_ptr(), None, ws_min.data_ptr(), need_e, None) == 0
        out_min, ws_d = up(b.pcm_image(fill=False)[:b.t.pcm_samples]), t.full((need_d,), 0xCD, dtype=t.uint8, device="cuda")
        assert dec(h, adx_min.data_ptr(), out_min.data_ptr(), ws_d.data_ptr(), need_d, S, None) == 0
        t.cuda.synchronize()
        b.check_adx(np.concatenate([adx_min.cpu().numpy(), np.full(EXTRA, JUNK, np.uint8)]), "at the minimum")
        b.check_pcm(np.concatenate([out_min.cpu().numpy(), np.full(EXTRA, SENTINEL, np.int16)]), "at the minimum")

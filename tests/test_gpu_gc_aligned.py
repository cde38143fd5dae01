"""Sets of GC-ADPCM files whose loops need the alignment re-encode, on the device (include/vgaudio_hip/gc_files_aligned.h):
vga_gcadpcm_align_channels_device_v on the packed rows of one set of files (tests/gc_aligned_cases.py: the smallest shapes at
which each branch can go wrong, the default multiple of 14 336 and one tail the encoder cuts in two pieces).  Every channel's
aligned ADPCM, PCM, seek table and loop context must be the oracle's gc_build_channel and what
vga_gcadpcm_build_channels_device writes for that file alone.  All buffers are larger than needed and full of junk, and every
byte outside the rows, tables and contexts is compared afterwards.  The header is outside the lists the older test files
enumerate, so this file carries its own table (CASES); tests/test_gc_aligned_host.py holds that table to the header."""
import ctypes as C

import numpy as np
import pytest

import gc_aligned_cases as ga
import gc_files_cases as gf
from test_gpu_device_streams import delay  # noqa: F401  (the calibrated GPU delay that makes a caller's stream busy)
from vgaudio_amd import _lib
from vgaudio_amd.dsp import DspFileSet
from vgaudio_amd.gcadpcm import AlignedFileSet

pytestmark = pytest.mark.gpu

# function of the header -> the tests below that call it
CASES = {
    "vga_gc_aligned_layout_for": ["test_object_numbers_are_the_host_layouts"],
    "vga_gc_aligned_create": ["test_chain_matches_oracle", "test_object_numbers_are_the_host_layouts"],
    "vga_gc_aligned_destroy": ["test_chain_matches_oracle"],
    "vga_gc_aligned_totals_of": ["test_object_numbers_are_the_host_layouts"],
    "vga_gc_aligned_offsets": ["test_object_numbers_are_the_host_layouts"],
    "vga_gc_aligned_ragged_in": ["test_object_numbers_are_the_host_layouts", "test_chain_matches_oracle"],
    "vga_gc_aligned_ragged_out": ["test_object_numbers_are_the_host_layouts", "test_rows_go_straight_into_the_brstm_writer"],
    "vga_gcadpcm_align_channels_device_v": [
        "test_chain_matches_oracle", "test_set_matches_the_per_file_call", "test_context_past_the_original_data",
        "test_a_set_without_alignment_is_the_plain_build", "test_a_set_in_which_every_file_needs_it", "test_bytes_do_not_depend_on_poison",
        "test_call_on_a_busy_stream", "test_two_calls_on_two_streams", "test_refused_buffers_launch_nothing",
        "test_rows_go_straight_into_the_brstm_writer", "test_build_files_returns_the_formats_channels"],
}

SENTINEL = 0x7777
JUNK = 0xEE
EXTRA = 64
POOL_STREAMS = 32                                                      # torch hands out this many streams, round robin


def torch():
    import torch as t
    return t


def L():
    return _lib.lib()


def dev(a):
    return torch().from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def junk(n, value=JUNK, dtype=np.uint8):
    return np.full(n + EXTRA, value, dtype)


def stream_ptr(stream=None):
    return C.c_void_p((stream if stream is not None else torch().cuda.current_stream()).cuda_stream)


# ---------------------------------------------------------------- the per-file call, computed once per list of files
_own = {}


def per_file(tuples, with_context=True):
    """vga_gcadpcm_build_channels_device on every file alone: per file, per channel {"out", "pcm", "seek", "ctx"}; the inputs are the
    oracle's encode of tests/gc_aligned_cases.py"""
    key = (tuple(tuples), with_context)
    if key in _own:
        return _own[key]
    t, out = torch(), []
    for tup, chans in zip(tuples, ga.reference(tuples)):
        f = ga.gc_file(*tup)
        p, nch, lay = f.channel, f.channels, ga.channel_layout(f)
        n_al, entries = lay.sample_count_aligned, lay.seek_table_entries
        in_bytes, out_bytes = ga.byte_count(p.sample_count), ga.byte_count(n_al)
        if p.sample_count == 0:                                        # nothing to read or write
            out.append([{"out": np.zeros(0, np.uint8), "pcm": np.zeros(0, np.int16), "seek": np.zeros(0, np.int16), "ctx": np.zeros(3, np.int16)}
                        for _ in range(nch)])
            continue
        in_pitch, out_pitch, pcm_pitch, seek_pitch = (max(ga.up(v, 16), 16) for v in (in_bytes, out_bytes, n_al, 2 * entries))
        rows = np.zeros((nch, in_pitch), np.uint8)
        for i, ch in enumerate(chans):
            rows[i, :in_bytes] = ch["adpcm"]
        d_in, d_coefs = dev(rows), dev(np.stack([ch["coefs"] for ch in chans]))
        d_out = t.full((nch, out_pitch), JUNK, dtype=t.uint8, device="cuda")
        d_pcm = t.full((nch, pcm_pitch), SENTINEL, dtype=t.int16, device="cuda")
        d_seek = t.full((nch, seek_pitch), SENTINEL, dtype=t.int16, device="cuda")
        d_ctx = t.full((nch * 3,), SENTINEL, dtype=t.int16, device="cuda")
        need = L().vga_gcadpcm_build_channels_workspace_bytes(nch, C.byref(p))
        ws = t.empty(need + 16, dtype=t.uint8, device="cuda")
        _lib.check(L().vga_gcadpcm_build_channels_device(d_in.data_ptr(), in_pitch, d_coefs.data_ptr(), nch, C.byref(p), d_out.data_ptr(), out_pitch,
                                                         d_pcm.data_ptr(), pcm_pitch, d_seek.data_ptr(), seek_pitch,
                                                         d_ctx.data_ptr() if with_context else None, ws.data_ptr(), need, None))
        t.cuda.synchronize()
        o, q, s, x = host(d_out), host(d_pcm), host(d_seek), host(d_ctx)
        out.append([{"out": o[i, :out_bytes].copy(), "pcm": q[i, :n_al].copy(), "seek": s[i, :2 * entries].copy(), "ctx": x[3 * i:3 * i + 3].copy()}
                    for i in range(nch)])
    _own[key] = out
    return out


# ---------------------------------------------------------------- one set and its junk-filled buffers
class Set:
    def __init__(self, tuples):
        self.tuples = list(tuples)
        self.files = ga.files_of(self.tuples)
        self.s = AlignedFileSet(self.files)
        self.m = ga.model(self.files)
        self.t = self.s.totals
        self.ref = [ch for f in ga.reference(self.tuples) for ch in f]
        self.pin, self.ain = self.s.offsets("in")
        self.pout, self.aout = self.s.offsets("out")
        self.nch = self.s.channels

    def close(self):
        torch().cuda.synchronize()
        self.s.close()

    def adpcm_image(self):
        img = junk(self.t.adpcm_bytes)
        for ch, at in zip(self.ref, self.ain):
            img[at:at + ch["adpcm"].size] = ch["adpcm"]
        return img

    def coefs(self):
        return np.stack([ch["coefs"] for ch in self.ref]).astype(np.int16).reshape(-1)

    def buffers(self, pcm=True, seek=True, ctx=True, ws_fill=0xCD):
        t = torch()
        return {"adpcm": dev(self.adpcm_image()), "coefs": dev(self.coefs()), "out": dev(junk(self.t.out_adpcm_bytes)),
                "pcm": dev(junk(self.t.out_pcm_samples, SENTINEL, np.int16)) if pcm else None,
                "seek": dev(junk(self.t.seek_shorts, SENTINEL, np.int16)) if seek else None,
                "ctx": dev(junk(self.nch * 3, SENTINEL, np.int16)) if ctx else None,
                "status": t.zeros(2, dtype=t.int32, device="cuda"), "ws": dev(junk(self.t.workspace_bytes, ws_fill))}

    def run(self, b, stream=None):
        self.s.align_channels(b["adpcm"], b["coefs"], b["out"], pcm=b["pcm"], seek=b["seek"], loop_context=b["ctx"], status=b["status"],
                              workspace=b["ws"], stream=stream)
        return b

    def check_rows(self, got, offsets, want, key, fill, what):
        own = np.zeros(got.size, bool)
        for c, (ch, at) in enumerate(zip(want, offsets)):
            w = ch[key]
            own[at:at + w.size] = True
            assert np.array_equal(got[at:at + w.size], w), (what, key, "channel", c, "file", self.m_file(c))
        assert np.all(got[~own] == fill), (what, key, "wrote outside the channels' own rows: a gap, the guard or the tail")

    def m_file(self, c):
        f = int(np.searchsorted(self.s.first_channel, c, side="right")) - 1
        return f, self.tuples[f]

    def check(self, b, what, want=None, ws_fill=0xCD):
        """want: per channel {"out", "pcm", "seek", "ctx"}; None: the oracle's"""
        want = self.ref if want is None else want
        assert np.array_equal(host(b["adpcm"]), self.adpcm_image()), "d_adpcm is an input"
        assert np.array_equal(host(b["coefs"]), self.coefs()), "d_coefs is an input"
        self.check_rows(host(b["out"]), self.aout, want, "out", JUNK, what)
        if b["pcm"] is not None:
            self.check_rows(host(b["pcm"]), self.pout, want, "pcm", SENTINEL, what)
        if b["seek"] is not None:
            self.check_rows(host(b["seek"]), self.s.seek_offsets, want, "seek", SENTINEL, what)
        if b["ctx"] is not None:
            ctx = host(b["ctx"])
            for c, ch in enumerate(want):
                assert np.array_equal(ctx[3 * c:3 * c + 3], ch["ctx"]), (what, "context", c, self.m_file(c))
            assert np.all(ctx[self.nch * 3:] == SENTINEL), what
        assert np.all(host(b["status"]) == 0)
        assert np.all(host(b["ws"])[self.t.workspace_bytes:] == ws_fill), (what, "wrote behind the workspace")


def flat(per_file_chans):
    return [ch for f in per_file_chans for ch in f]


def run_set(tuples, what, want=None, ctx=True):
    a = Set(tuples)
    try:
        want = a.ref if want is None else want
        full = a.run(a.buffers(ctx=ctx))
        no_pcm, no_seek = a.run(a.buffers(pcm=False, ctx=ctx)), a.run(a.buffers(seek=False, ctx=ctx))
        no_ctx = a.run(a.buffers(ctx=False))
        torch().cuda.synchronize()
        a.check(full, (what, "all outputs"), want)
        a.check(no_pcm, (what, "d_pcm_out NULL"), want)
        a.check(no_seek, (what, "d_seek_out NULL"), want)
        a.check(no_ctx, (what, "context NULL"), want)
    finally:
        a.close()


# ---------------------------------------------------------------- 1. the chain against the oracle
def test_chain_matches_oracle():
    """vga_gcadpcm_coefs_device_v -> vga_gcadpcm_encode_device_v on ragged_in -> the new call; then the call on the oracle's rows
    with each optional output left out"""
    t = torch()
    ref = ga.reference(ga.SET)
    assert all(ch["rc"] == 0 for f in ref for ch in f)
    changed = sum(any(not np.array_equal(ch["pcm"][:tup[4]], ch["plain"][:tup[4]]) for ch in f)
                  for tup, f in zip(ga.SET, ref) if tup in ga.NEEDS)
    assert changed >= 9, "the re-encode changes the PCM below the loop end: copy-and-append is not the reference"
    a = Set(ga.SET)
    try:
        pcm = junk(a.t.pcm_samples, 0, np.int16)
        for ch, at in zip(a.ref, a.pin):
            pcm[at:at + ch["x"].size] = ch["x"]
        b = a.buffers()
        d_pcm = dev(pcm)
        b["adpcm"], b["coefs"] = dev(junk(a.t.adpcm_bytes)), t.zeros(a.nch * 16, dtype=t.int16, device="cuda")
        cws = t.empty(max(L().vga_gcadpcm_ragged_coefs_workspace_bytes(a.s.ragged_in), 16), dtype=t.uint8, device="cuda")
        _lib.check(L().vga_gcadpcm_coefs_device_v(a.s.ragged_in, d_pcm.data_ptr(), b["coefs"].data_ptr(), cws.data_ptr(), cws.numel(), stream_ptr()))
        _lib.check(L().vga_gcadpcm_encode_device_v(a.s.ragged_in, d_pcm.data_ptr(), b["coefs"].data_ptr(), None, None, b["adpcm"].data_ptr(), stream_ptr()))
        a.run(b)
        t.cuda.synchronize()
        a.check(b, "chain")
    finally:
        a.close()
    run_set(ga.SET, "oracle rows")


# ---------------------------------------------------------------- 2. the per-file call
def test_set_matches_the_per_file_call():
    own = flat(per_file(ga.SET))
    for c, (o, r) in enumerate(zip(own, flat(ga.reference(ga.SET)))):     # (the per-file call is the oracle's, too)
        assert all(np.array_equal(o[k], r[k]) for k in ("out", "pcm", "seek", "ctx")), c
    a = Set(ga.SET)
    try:
        b = a.run(a.buffers())
        torch().cuda.synchronize()
        a.check(b, "per-file", own)
    finally:
        a.close()


# ---------------------------------------------------------------- 3. the aligned loop start past the original data
def test_context_past_the_original_data():
    t = torch()
    assert all(ch["rc"] == -2 for f in ga.reference(ga.REFUSED_SET) for ch in f)
    tuples = ga.SET[:2] + ga.REFUSED_SET
    a = Set(tuples)
    try:
        b = a.buffers()
        with pytest.raises(_lib.ArgumentOutOfRangeError, match=r"file 2\b"):
            a.run(b)
        t.cuda.synchronize()
        assert np.all(host(b["out"]) == JUNK) and np.all(host(b["pcm"]) == SENTINEL) and np.all(host(b["seek"]) == SENTINEL)
        assert np.all(host(b["ctx"]) == SENTINEL) and np.all(host(b["ws"]) == 0xCD)
    finally:
        a.close()
    run_no_ctx = flat(per_file(tuples, with_context=False))
    a = Set(tuples)
    try:
        for kw in ({}, {"pcm": False}, {"seek": False}):
            b = a.run(a.buffers(ctx=False, **kw))
            t.cuda.synchronize()
            a.check(b, ("no context", kw), run_no_ctx)
    finally:
        a.close()


# ---------------------------------------------------------------- 4. nothing to align
def encode_pieces(reset=True):
    out8 = (C.c_ulonglong * 8)()
    assert L().vga_testing_gc_encode_stats(out8, int(reset)) == 0
    return int(out8[6])


def test_a_set_without_alignment_is_the_plain_build():
    """the files of tests/gc_files_cases.py: outputs are vga_gcadpcm_build_channels_device_v's, the output rows the input rows, and
    the encoder is not launched"""
    t = torch()
    tuples = [f + (0,) for f in gf.FILES]
    a = Set(tuples)
    plain = DspFileSet(a.files, None)
    try:
        assert a.t.aligned_channels == 0 and (a.t.out_pcm_samples, a.t.out_adpcm_bytes) == (a.t.pcm_samples, a.t.adpcm_bytes)
        assert list(a.aout) == list(a.ain) and list(a.pout) == list(a.pin) and list(a.s.seek_offsets) == list(plain.seek_offsets)
        b = a.buffers()
        want = {"pcm": dev(junk(a.t.pcm_samples, SENTINEL, np.int16)), "seek": dev(junk(a.t.seek_shorts, SENTINEL, np.int16)),
                "ctx": dev(junk(a.nch * 3, SENTINEL, np.int16))}
        ws = dev(junk(plain.totals.build_workspace_bytes))
        plain.build_channels(b["adpcm"], b["coefs"], pcm=want["pcm"], seek=want["seek"], loop_context=want["ctx"], workspace=ws)
        encode_pieces()
        a.run(b)
        assert encode_pieces() == 0, "the encoder ran in a set without tails"
        for k in want:
            assert np.array_equal(host(b[k]), host(want[k])), k
        assert np.array_equal(host(b["out"]), a.adpcm_image())        # rows, gaps and guard alike: both were filled with the same junk
        assert np.all(host(b["ws"]) == 0xCD), "the caller takes the PCM: the workspace is not needed"
        a.check(b, "no alignment")
        # into the workspace when the caller does not take the PCM; nothing at all when nothing reads it
        b2 = a.run(a.buffers(pcm=False))
        t.cuda.synchronize()
        a.check(b2, "no alignment, PCM in the workspace")
        loops0 = Set([(2, 100, 1, 0, 57, 14, 14), (1, 30, 0, 0, 0, 0, 0)])
        try:
            b3 = loops0.buffers(pcm=False, seek=False)
            loops0.s.align_channels(b3["adpcm"], b3["coefs"], b3["out"], loop_context=b3["ctx"])      # no workspace at all
            t.cuda.synchronize()
            assert np.all(host(b3["ctx"])[:9] == 0)
            b3["status"].zero_()
            loops0.check(b3, "no decode")
        finally:
            loops0.close()
    finally:
        plain.close()
        a.close()


# ---------------------------------------------------------------- 5. every file needs it
def test_a_set_in_which_every_file_needs_it():
    a = Set(ga.NEEDS)
    try:
        assert a.t.aligned_channels == a.t.channels
    finally:
        a.close()
    encode_pieces()
    run_set(ga.NEEDS, "every file")
    assert encode_pieces() > 0, "the encoder did not run"


def test_object_numbers_are_the_host_layouts():
    a = Set(ga.SET)
    try:
        fc, so, tot = AlignedFileSet.layout(a.files)
        assert all(getattr(tot, f) == getattr(a.t, f) for f, _ in tot._fields_)
        assert np.array_equal(fc, a.s.first_channel) and np.array_equal(so, a.s.seek_offsets)
        fc2, so2 = np.zeros(tot.files, np.int32), np.zeros(tot.channels, np.int64)
        _lib.check(L().vga_gc_aligned_offsets(a.s._h, fc2.ctypes.data_as(C.POINTER(C.c_int)), so2.ctypes.data_as(C.POINTER(C.c_int64))))
        assert np.array_equal(fc2, fc) and np.array_equal(so2, so)
        t2 = _lib.GcAlignedTotalsC()
        _lib.check(L().vga_gc_aligned_totals_of(a.s._h, C.byref(t2)))
        assert all(getattr(t2, f) == getattr(tot, f) for f, _ in tot._fields_)
        # the borrowed batches are the ones vga_gcadpcm_ragged_create makes of the respective counts
        for r, pcm_samples, adpcm_bytes, key in ((L().vga_gc_aligned_ragged_in(a.s._h), tot.pcm_samples, tot.adpcm_bytes, "in"),
                                                 (L().vga_gc_aligned_ragged_out(a.s._h), tot.out_pcm_samples, tot.out_adpcm_bytes, "out")):
            assert r and L().vga_gcadpcm_ragged_channels(r) == tot.channels
            assert L().vga_gcadpcm_ragged_pcm_samples(r) == pcm_samples and L().vga_gcadpcm_ragged_adpcm_bytes(r) == adpcm_bytes
            po_, ao_ = a.s.offsets(key)
            assert list(po_) == a.m[key + "_pcm_off"] and list(ao_) == a.m[key + "_adpcm_off"]
        sb = a.t.workspace_bytes - a.m["scratch_at"]
        assert a.t.workspace_bytes == ga.model(a.files, lambda n: sb)["workspace"]
    finally:
        a.close()


# ---------------------------------------------------------------- 6. poison mode
@pytest.mark.parametrize("value", [0xA5, 0xFF])
def test_bytes_do_not_depend_on_poison(value):
    old = L().vga_testing_poison_allocations(value)
    try:
        a = Set(ga.SET)                                                # (created under the mode: its tables are poisoned first)
        try:
            b = a.run(a.buffers(ws_fill=value ^ 0x3C))
            b2 = a.run(a.buffers(pcm=False, ws_fill=value))
            torch().cuda.synchronize()
            a.check(b, ("poison", value), ws_fill=value ^ 0x3C)
            a.check(b2, ("poison", value, "no PCM"), ws_fill=value)
        finally:
            a.close()
    finally:
        torch().cuda.synchronize()
        L().vga_testing_poison_allocations(old if old >= 0 else -1)


# ---------------------------------------------------------------- 7. a busy caller stream
_streams = []


def some_streams(n):
    """Streams for this file, taken once and so that the files that run after it find torch's stream pool as they would without
    it (tests/test_gpu_gc_files.py: one_stream): one whole turn of the pool with the imported `delay` fixture's, every stream
    used once, in order."""
    t = torch()
    if not _streams:
        _streams.extend(t.cuda.Stream() for _ in range(POOL_STREAMS - 1))
        for s in _streams:
            with t.cuda.stream(s):
                t.zeros(1, device="cuda")
        t.cuda.synchronize()
    return _streams[:n]


def test_call_on_a_busy_stream(delay):  # noqa: F811
    """the call queued behind a delay on the caller's stream: it does not wait for it, and it is ordered after it -- its input rows
    are written on the same stream after the delay"""
    t = torch()
    cycles, ms = delay
    a = Set(ga.SET)
    try:
        (S,) = some_streams(1)
        image = dev(a.adpcm_image())
        with t.cuda.stream(S):
            for busy in (False, True):                                 # (warm first: every kernel has run once)
                b = a.buffers(pcm=False)
                b["adpcm"] = dev(junk(a.t.adpcm_bytes, 0))
                S.synchronize()
                if busy:
                    t.cuda._sleep(cycles)
                b["adpcm"].copy_(image, non_blocking=True)             # the rows arrive behind the delay
                a.run(b, stream=S)
                if busy:
                    assert not S.query(), "the caller's stream was idle when the call returned (it waited for it)"
        S.synchronize()
        a.check(b, "busy stream")
    finally:
        a.close()


def test_two_calls_on_two_streams():
    """one object, two streams, two workspaces"""
    t = torch()
    a = Set(ga.SET)
    try:
        S1, S2 = some_streams(2)
        b1, b2 = a.buffers(), a.buffers(pcm=False, ws_fill=0x11)
        t.cuda.synchronize()
        a.run(b1, stream=S1)
        a.run(b2, stream=S2)
        S1.synchronize()
        S2.synchronize()
        a.check(b1, "stream 1")
        a.check(b2, "stream 2", ws_fill=0x11)
    finally:
        a.close()


# ---------------------------------------------------------------- 8. refused buffers
def test_refused_buffers_launch_nothing():
    t = torch()
    ARG = _lib.VGA_ERR_ARGUMENT
    a = Set(ga.SET)
    try:
        h, need = a.s._h, a.t.workspace_bytes
        b = a.buffers()
        A, K, O, P, S, X, W = (b[k].data_ptr() for k in ("adpcm", "coefs", "out", "pcm", "seek", "ctx", "ws"))
        call = L().vga_gcadpcm_align_channels_device_v
        assert call(h, A + 8, K, O, P, S, X, None, W, need, None) == ARG
        assert call(h, A, K, O + 8, P, S, X, None, W, need, None) == ARG
        assert call(h, A, K, O, P + 8, S, X, None, W, need, None) == ARG
        assert call(h, A, K, O, P, S + 8, X, None, W, need, None) == ARG
        assert call(h, A, K, O, P, S, X, None, W + 8, need, None) == ARG
        assert call(h, A, K, O, P, S, X, None, W, need - 1, None) == ARG
        assert call(h, A, K, O, P, S, X, None, None, need, None) == ARG
        assert call(h, None, K, O, P, S, X, None, W, need, None) == ARG and call(h, A, None, O, P, S, X, None, W, need, None) == ARG
        assert call(h, A, K, None, P, S, X, None, W, need, None) == ARG
        t.cuda.synchronize()
        assert np.all(host(b["out"]) == JUNK) and np.all(host(b["pcm"]) == SENTINEL) and np.all(host(b["seek"]) == SENTINEL)
        assert np.all(host(b["ctx"]) == SENTINEL) and np.all(host(b["ws"]) == 0xCD)
        # exactly at the minimum: buffers of the totals' sizes
        m = {"adpcm": dev(a.adpcm_image()[:a.t.adpcm_bytes]), "out": dev(junk(a.t.out_adpcm_bytes)[:a.t.out_adpcm_bytes]),
             "pcm": dev(junk(a.t.out_pcm_samples, SENTINEL, np.int16)[:a.t.out_pcm_samples]),
             "seek": dev(junk(a.t.seek_shorts, SENTINEL, np.int16)[:a.t.seek_shorts]), "ws": dev(junk(need, 0xCD)[:need])}
        assert call(h, m["adpcm"].data_ptr(), K, m["out"].data_ptr(), m["pcm"].data_ptr(), m["seek"].data_ptr(), X, None, m["ws"].data_ptr(), need, None) == 0
        t.cuda.synchronize()
        pad = lambda v, fill: t.cat([v, t.full((EXTRA,), fill, dtype=v.dtype, device="cuda")])
        a.check({"adpcm": pad(m["adpcm"], JUNK), "coefs": b["coefs"], "out": pad(m["out"], JUNK), "pcm": pad(m["pcm"], SENTINEL),
                 "seek": pad(m["seek"], SENTINEL), "ctx": b["ctx"], "status": b["status"], "ws": pad(m["ws"], 0xCD)}, "at the minimum")
    finally:
        a.close()


# ---------------------------------------------------------------- 9. the consumer
def test_rows_go_straight_into_the_brstm_writer():
    """the rows of the output batch, the packed seek tables and the contexts of one stereo file are what vga_nwstm_write_device takes:
    the image is the one the per-file route (vga_gcadpcm_build_channels_device, then the same writer) produces"""
    t = torch()
    nch, n, ls, le = 2, 100, 15, 57
    p = _lib.NwParamsC()
    p.target, p.sample_rate, p.sample_count, p.looping, p.loop_start, p.loop_end = 0, ga.RATE, n, 1, ls, le
    p.samples_per_interleave, p.samples_per_seek_table_entry, p.loop_point_alignment, p.endianness = 14, 14, 14, -1
    lay = _lib.NwLayoutC()
    _lib.check(L().vga_nwstm_layout_for(C.byref(p), nch, C.byref(lay)))
    ch = lay.channel
    stereo = (nch, ch.sample_count, ch.looping, ch.loop_start, ch.loop_end, ch.samples_per_seek_table_entry, ch.loop_alignment_multiple)
    assert stereo == ga.looping((2, 100, 15, 57, 14, 14)) and lay.alignment_needed
    tuples = [ga.looping(ga.LOOPING[6]), stereo, ga.looping(ga.LOOPING[0])]
    a = Set(tuples)
    try:
        b = a.run(a.buffers())
        first = int(a.s.first_channel[1])
        assert first == 1 and L().vga_gc_aligned_ragged_out(a.s._h)
        pitch, seek_pitch = int(a.aout[first + 1] - a.aout[first]), int(a.s.seek_offsets[first + 1] - a.s.seek_offsets[first])
        assert lay.channel_adpcm_bytes == ga.byte_count(70) <= pitch and 2 * lay.channel_seek_entries <= seek_pitch
        write = L().vga_nwstm_write_device
        image = t.full((lay.file_size + 16,), JUNK, dtype=t.uint8, device="cuda")
        _lib.check(write(C.byref(p), nch, 1, None, b["out"].data_ptr() + int(a.aout[first]), pitch, lay.channel_adpcm_bytes,
                         b["coefs"].data_ptr() + 32 * first, None, None, b["ctx"].data_ptr() + 6 * first,
                         b["seek"].data_ptr() + 2 * int(a.s.seek_offsets[first]), seek_pitch, lay.channel_seek_entries, image.data_ptr(),
                         ga.up(lay.file_size, 16), stream_ptr()))
        own = per_file(tuples)[1]
        rows, seek = np.stack([c["out"] for c in own]), np.stack([c["seek"] for c in own])
        d_rows, d_seek, d_ctx = dev(rows), dev(seek), dev(np.concatenate([c["ctx"] for c in own]))
        d_coefs = dev(np.stack([c["coefs"] for c in ga.reference(tuples)[1]]))
        want = t.full((lay.file_size + 16,), JUNK, dtype=t.uint8, device="cuda")
        _lib.check(write(C.byref(p), nch, 1, None, d_rows.data_ptr(), rows.shape[1], lay.channel_adpcm_bytes, d_coefs.data_ptr(), None, None,
                         d_ctx.data_ptr(), d_seek.data_ptr(), seek.shape[1], lay.channel_seek_entries, want.data_ptr(), ga.up(lay.file_size, 16),
                         stream_ptr()))
        t.cuda.synchronize()
        got, want = host(image), host(want)
        assert np.array_equal(got, want) and np.all(got[lay.file_size:] == JUNK) and not np.all(got[:lay.file_size] == JUNK)
        assert got[:4].tobytes() == b"RSTM"
        a.check(b, "consumer")
    finally:
        a.close()


# ---------------------------------------------------------------- 10. the Python mirror
def test_build_files_returns_the_formats_channels():
    """gcadpcm.build_files -- upload, coefficients, encode, align on the device, one download -- gives per file what
    GcAdpcmFormat().EncodeFromPcm16(file)._clone(alignmentMultiple=, samplesPerSeekTableEntry=) holds"""
    from vgaudio_amd import gcadpcm
    pcm = ga.source_pcm()
    shapes = [(2, 1400, (15, 1000), 14, 14), (1, 3000, None, 0x3800, 0x3800), (3, 29, (2, 20), 4, 5)]
    files, c = [], 0
    for nch, n, loop, _, _ in shapes:
        f = gcadpcm.Pcm16Format([pcm[(c + i) % 64, :n] for i in range(nch)], 22050 + 1000 * nch)
        if loop:
            f.WithLoop(True, *loop)
        files.append(f)
        c += nch
    got = gcadpcm.build_files(files, [(m, e) for _, _, _, m, e in shapes])
    for k, (f, (_, _, _, m, e), g) in enumerate(zip(files, shapes, got)):
        want = gcadpcm.GcAdpcmFormat().EncodeFromPcm16(f)._clone(alignmentMultiple=m, samplesPerSeekTableEntry=e)
        assert g["sample_count"] == want.SampleCount and len(g["adpcm"]) == want.ChannelCount
        for i, chan in enumerate(want.Channels):
            assert np.array_equal(g["adpcm"][i], chan.GetAdpcmAudio()), ("file", k, "channel", i)
            assert np.array_equal(g["seek"][i], chan.GetSeekTable()), ("file", k, "channel", i)
            lc = chan.LoopContext
            assert list(g["context"][i]) == [lc.PredScale, lc.Hist1, lc.Hist2], ("file", k, "channel", i)
            assert np.array_equal(g["coefs"][i], chan.Coefs)
    assert gcadpcm.build_files([], []) == []

"""Looping streams in the packed HCA encode (include/vgaudio_hip_files/hca_ragged_loops.h): vga_hca_encode_loops_device_v on the
case objects of tests/hca_loop_cases.py -- loop cases interleaved with plain streams, per shape class -- against the CPU oracle
on the whole file and against one vga_hca_encode_device call per stream; nothing outside a stream's own frames may change.  All
buffers are larger than needed and full of junk.  Then the two callers of the same tables: vga_hca_encode_batch_v, whose looping
streams now bucket by shape (vga_testing_hca_encode_v_stats), and hca.write_files.  This file carries its own table (CASES) of
which test exercises which function of the header; tests/test_hca_ragged_loops_host.py holds that table to the header."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import hca_loop_cases as lc
from oracle import pyoracle as po
from test_gpu_device_streams import delay  # noqa: F401  (the calibrated GPU delay that makes a caller's stream busy)
from vgaudio_amd import _lib, crihca, hca
from vgaudio_amd.crihca import RaggedHca

pytestmark = pytest.mark.gpu

# function of the header -> the tests below that call it
CASES = {
    "vga_hca_loop_may_read_tail": ["test_encode_matches_the_oracle_on_the_whole_file", "test_write_files_groups_looping_files"],
    "vga_hca_encode_loops_device_v": ["test_encode_matches_the_oracle_on_the_whole_file", "test_encode_matches_one_call_per_stream",
                                      "test_plain_streams_are_what_the_older_call_writes", "test_bytes_do_not_depend_on_poison_or_run_length",
                                      "test_round_trip_on_a_busy_stream_and_two_streams_at_once", "test_refused_layouts_launch_nothing",
                                      "test_write_files_groups_looping_files"],
}

SENTINEL = 0x7777
JUNK = 0xEE
EXTRA = 64
NAMES = ["mono", "stereo", "six"]


def torch():
    import torch as t
    return t


def L():
    return _lib.lib()


def up(a):
    return torch().from_numpy(np.ascontiguousarray(a)).cuda()


def own_encode(s, pcm_length=None):
    """one vga_hca_encode_device call for the stream, its rows pcm_length long (default: HcaInfo.sample_count)"""
    h, t = s.info, torch()
    length = h.sample_count if pcm_length is None else pcm_length
    n = max(length, 1)
    pcm = t.zeros((h.channel_count, n), dtype=t.int16, device="cuda")
    if length:
        pcm[:, :length] = up(s.pcm[:, :length])
    pitch = (h.frame_count * h.frame_size + 8 + 3) // 4 * 4
    frames, st = t.zeros(pitch, dtype=t.uint8, device="cuda"), t.zeros(1, dtype=t.int32, device="cuda")
    _lib.check(L().vga_hca_encode_device(pcm.data_ptr(), h.channel_count * n, n, 1, length, C.byref(h), frames.data_ptr(), pitch,
                                         st.data_ptr(), None))
    t.cuda.synchronize()
    assert int(st.item()) == 0
    return frames.cpu().numpy()[:h.frame_count * h.frame_size]


@pytest.fixture(scope="module")
def classes():
    return lc.classes()


@pytest.fixture(scope="module")
def own(classes):
    """every stream's frames from its own vga_hca_encode_device call with pcm_length = sample_count: computed once, shared"""
    return {name: [own_encode(s) for s in streams] for name, streams in classes.items()}


class Batch:
    """a ragged object over `streams` and junk-filled packed buffers on the device"""

    def __init__(self, streams, want):
        self.streams, self.want = streams, want
        self.r = RaggedHca([s.info for s in streams])
        self.t, self.fo, self.ro = self.r.totals, self.r.frame_offsets, self.r.pcm_row_offsets
        self.rows = [(s, c) for s in streams for c in range(s.info.channel_count)]

    def close(self):
        self.r.close()

    def frames_image(self, fill=False):
        img = np.full(self.t.frame_bytes + EXTRA, JUNK, np.uint8)
        if fill:
            for w, at in zip(self.want, self.fo):
                img[at:at + w.size] = w
        return img

    def pcm_image(self, fill=True):
        img = np.full(self.t.pcm_samples + EXTRA, SENTINEL, np.int16)
        if fill:
            for (s, c), at in zip(self.rows, self.ro):
                img[at:at + s.info.sample_count] = s.pcm[c, :s.info.sample_count]
        return img

    def status(self):
        return torch().zeros(len(self.streams) + 1, dtype=torch().int32, device="cuda")

    def encode(self, stream=None):
        pcm, frames, st = up(self.pcm_image()), up(self.frames_image()), self.status()
        self.r.encode_loops_device(pcm, frames, st, stream=stream)
        return pcm, frames, st

    def check_frames(self, got, what):
        """got: host image after an encode: every stream's frames those of its own call, everything else untouched"""
        own = np.zeros(got.size, bool)
        for i, (s, w, at) in enumerate(zip(self.streams, self.want, self.fo)):
            own[at:at + w.size] = True
            assert w.size == s.info.frame_count * s.info.frame_size
            bad = np.flatnonzero(got[at:at + w.size] != w)
            assert bad.size == 0, (what, "stream", i, (s.n, s.loop), "first differing frame", int(bad[0]) // s.info.frame_size)
        assert np.all(got[~own] == JUNK), (what, "wrote outside the streams' own frames")


@contextlib.contextmanager
def batch_of(streams, want):
    b = Batch(streams, want)
    try:
        yield b
    finally:
        torch().cuda.synchronize()
        b.close()


# ---------------------------------------------------------------- the contract
@pytest.mark.parametrize("name", NAMES)
def test_encode_matches_one_call_per_stream(classes, own, name):
    with batch_of(classes[name], own[name]) as b:
        pcm, frames, st = b.encode()
        torch().cuda.synchronize()
        assert np.all(st.cpu().numpy() == 0)
        b.check_frames(frames.cpu().numpy(), name)
        assert np.array_equal(pcm.cpu().numpy(), b.pcm_image()), "d_pcm is an input"


@pytest.mark.parametrize("name", NAMES)
def test_encode_matches_the_oracle_on_the_whole_file(classes, own, name):
    streams = classes[name]
    flagged = [s for s in streams if s.may_read_tail]
    assert [s.may_read_tail for s in streams if s.info.looping] == [False, False, False, False, True, True, True, False, True]
    assert [s.row_is_the_file for s in flagged] == [True, True, True, False]
    with batch_of(streams, own[name]) as b:
        _, frames, st = b.encode()
        torch().cuda.synchronize()
        got = frames.cpu().numpy()
        assert np.all(st.cpu().numpy() == 0)
    for i, (s, at) in enumerate(zip(streams, b.fo)):
        mine = got[at:at + s.frames.size]
        if s.row_is_the_file:
            assert np.array_equal(mine, s.frames), (name, "stream", i, (s.n, s.loop))
        else:       # the file's audio behind SampleCount reaches the oracle's frames: the per-file call with the file's length has it
            assert not np.array_equal(mine, s.frames)
            assert np.array_equal(own_encode(s, pcm_length=s.n), s.frames), (name, "stream", i)


@pytest.mark.parametrize("name", NAMES)
def test_plain_streams_are_what_the_older_call_writes(classes, own, name):
    keep = [i for i, s in enumerate(classes[name]) if not s.info.looping]
    streams, want = [classes[name][i] for i in keep], [own[name][i] for i in keep]
    with batch_of(streams, want) as b:
        pcm, old, st = up(b.pcm_image()), up(b.frames_image()), b.status()
        b.r.encode_device(pcm, old, st)
        _, new, st2 = b.encode()                                      # an object without loops may use either call
        torch().cuda.synchronize()
        assert np.all(st.cpu().numpy() == 0) and np.all(st2.cpu().numpy() == 0)
        assert np.array_equal(old.cpu().numpy(), new.cpu().numpy())
        b.check_frames(new.cpu().numpy(), name)


# ---------------------------------------------------------------- poison mode, frames per run
@pytest.mark.parametrize("mode", ["poison-a5", "poison-ff", "run-1", "run-3", "run-16"])
def test_bytes_do_not_depend_on_poison_or_run_length(classes, own, mode):
    kind, _, value = mode.partition("-")
    if kind == "poison":
        old = L().vga_testing_poison_allocations(int(value, 16))
    else:
        old = L().vga_testing_hca_frames_per_group_this_thread(int(value))
    try:
        for name, streams in classes.items():
            with batch_of(streams, own[name]) as b:                   # (created under the mode: its tables are poisoned first)
                for call in range(2):                                 # the second call reuses the tables the first one made
                    _, frames, st = b.encode()
                    torch().cuda.synchronize()
                    assert np.all(st.cpu().numpy() == 0)
                    b.check_frames(frames.cpu().numpy(), (mode, name, call))
    finally:
        torch().cuda.synchronize()
        if kind == "poison":
            L().vga_testing_poison_allocations(old if old >= 0 else -1)
        else:
            L().vga_testing_hca_frames_per_group_this_thread(old)


# ---------------------------------------------------------------- a busy caller stream, two streams at once
def test_round_trip_on_a_busy_stream_and_two_streams_at_once(classes, own, delay):  # noqa: F811
    t = torch()
    cycles, ms = delay
    streams = classes["stereo"]
    with batch_of(streams, own["stereo"]) as b:
        A, B = t.cuda.Stream(), t.cuda.Stream()
        out = {}
        for name, S, busy in (("warm", A, False), ("A", A, True), ("B", B, False)):
            with t.cuda.stream(S):
                pcm_in, frames = up(b.pcm_image()), up(b.frames_image())
                pcm_out = up(b.pcm_image(fill=False))
                ws = t.full((b.t.decode_workspace_bytes + EXTRA,), 0xCD, dtype=t.uint8, device="cuda")
                st = b.status()
                if busy:
                    t.cuda._sleep(cycles)
            b.r.encode_loops_device(pcm_in, frames, st, stream=S)     # encode, then decode what it wrote: no host synchronisation
            b.r.decode_device(frames, pcm_out, ws, st, stream=S)
            if busy:
                assert not S.query(), "the caller's stream was idle when the calls returned (they waited for it)"
            out[name] = (frames, pcm_out, st, pcm_in, ws)
            if name == "warm":
                S.synchronize()
        B.synchronize()
        A.synchronize()
        for name in ("A", "B"):
            frames, pcm_out, st = out[name][:3]
            assert np.all(st.cpu().numpy() == 0)
            b.check_frames(frames.cpu().numpy(), name)
            got = pcm_out.cpu().numpy()
            owned = np.zeros(got.size, bool)
            for (s, c), at in zip(b.rows, b.ro):
                n = s.info.sample_count
                owned[at:at + n] = True
                if s.row_is_the_file:                                 # (the oracle's decode is of the oracle's frames)
                    assert np.array_equal(got[at:at + n], s.want[c]), (name, (s.n, s.loop), c)
            assert np.all(got[~owned] == SENTINEL)
        assert t.equal(out["A"][0], out["B"][0]) and t.equal(out["A"][1], out["B"][1])


# ---------------------------------------------------------------- refused layouts
def test_refused_layouts_launch_nothing(classes, own):
    t = torch()
    with batch_of(classes["stereo"], own["stereo"]) as b:
        pcm = up(np.concatenate([b.pcm_image(), np.full(16, SENTINEL, np.int16)]))
        out = up(np.concatenate([b.frames_image(), np.full(16, JUNK, np.uint8)]))
        st = b.status()
        h, enc = b.r._h, L().vga_hca_encode_loops_device_v
        assert enc(h, pcm.data_ptr() + 8, out.data_ptr(), st.data_ptr(), None) == _lib.VGA_ERR_ARGUMENT
        assert b"vga_hca_encode_loops_device_v" in L().vga_last_error()
        assert enc(h, pcm.data_ptr(), out.data_ptr() + 2, st.data_ptr(), None) == _lib.VGA_ERR_ARGUMENT
        assert enc(h, None, out.data_ptr(), st.data_ptr(), None) == _lib.VGA_ERR_ARGUMENT
        assert enc(h, pcm.data_ptr(), None, st.data_ptr(), None) == _lib.VGA_ERR_ARGUMENT
        assert enc(h, pcm.data_ptr(), out.data_ptr(), None, None) == _lib.VGA_ERR_ARGUMENT
        assert enc(None, pcm.data_ptr(), out.data_ptr(), st.data_ptr(), None) == _lib.VGA_ERR_ARGUMENT
        t.cuda.synchronize()
        assert np.all(out.cpu().numpy() == JUNK) and np.all(st.cpu().numpy() == 0)
        assert np.array_equal(pcm.cpu().numpy()[:-16], b.pcm_image())
    # an info that does not describe its PCM is refused as the per-stream call refuses it
    bad = _lib.HcaInfoC.from_buffer_copy(classes["stereo"][1].info)
    bad.appended_samples += 4096
    r = RaggedHca([classes["stereo"][0].info, bad])
    try:
        pcm = t.zeros(r.totals.pcm_samples + 16, dtype=t.int16, device="cuda")
        out = t.full((r.totals.frame_bytes + 16,), JUNK, dtype=t.uint8, device="cuda")
        st = t.zeros(3, dtype=t.int32, device="cuda")
        assert L().vga_hca_encode_loops_device_v(r._h, pcm.data_ptr(), out.data_ptr(), st.data_ptr(), None) == _lib.VGA_ERR_ARGUMENT
        t.cuda.synchronize()
        assert np.all(out.cpu().numpy() == JUNK)
    finally:
        r.close()


# ---------------------------------------------------------------- vga_hca_encode_batch_v: looping streams bucket by shape
def test_host_batch_puts_looping_streams_of_one_shape_into_one_group():
    loops = lc.LOOP_CASES + lc.TAIL_READERS[1:]                       # 12 different loops, the tail readers among them
    assert len(loops) == 12 == len(set(loops))
    streams = [lc.Stream(2, c[0], 40 + k, loop=c[1:]) for k, c in enumerate(loops)]
    streams += [lc.Stream(2, n, 60 + k) for k, n in enumerate((500, 0, 7000, 23000))]
    order = np.random.default_rng(5).permutation(len(streams))
    streams = [streams[i] for i in order]
    files = [crihca.Pcm16Format(list(s.pcm), 48000) for s in streams]
    for f, s in zip(files, streams):
        if s.loop:
            f.Looping, f.LoopStart, f.LoopEnd = True, s.loop[0], s.loop[1]
    got = crihca.encode_files(files)
    v = (C.c_longlong * 4)()
    assert L().vga_testing_hca_encode_v_stats(v, 4) == 4
    for k, (g, s) in enumerate(zip(got, streams)):                    # the host call sees the whole file: the oracle's, always
        assert g.Hca.FrameCount == s.info.frame_count
        assert np.array_equal(np.asarray(g.AudioData).reshape(-1), s.frames), ("stream", k, (s.n, s.loop))
    # one group for the twelve looping streams (a group per loop before), one for the plain ones
    assert (v[0], v[1]) == (16, 2), list(v)
    # a chunk is a bucket of similar lengths and one launch: fewer of them than looping streams alone (a launch per loop before)
    assert v[3] == v[2] < 12, list(v)


# ---------------------------------------------------------------- hca.write_files
def per_file_image(f, info, key):
    """the per-file route: vga_hca_encode_device on the whole file, vga_hca_crypt_device, vga_hca_write_device"""
    t = torch()
    n, nch = f.SampleCount, f.ChannelCount
    pcm = t.zeros((nch, max(n, 1)), dtype=t.int16, device="cuda")
    if n:
        pcm[:, :n] = up(np.stack([np.asarray(c, np.int16) for c in f.Channels]))
    nb = info.frame_count * info.frame_size
    pitch = (nb + 8 + 3) // 4 * 4
    d, st = t.zeros(pitch, dtype=t.uint8, device="cuda"), t.zeros(1, dtype=t.int32, device="cuda")
    _lib.check(L().vga_hca_encode_device(pcm.data_ptr(), nch * max(n, 1), max(n, 1), 1, n, C.byref(info), d.data_ptr(), pitch, st.data_ptr(), None))
    if key is not None:
        table = np.ascontiguousarray(key.EncryptionTable, dtype=np.uint8)
        _lib.check(L().vga_hca_crypt_device(d.data_ptr(), pitch, 1, info.frame_count, info.frame_size,
                                            table.ctypes.data_as(C.POINTER(C.c_uint8)), None))
    size = info.header_size + nb
    out = t.full((size + 16,), JUNK, dtype=t.uint8, device="cuda")
    _lib.check(L().vga_hca_write_device(C.byref(info), d.data_ptr(), pitch, 1, None, 1.0, key.KeyType if key is not None else 0,
                                        int(key is not None), out.data_ptr(), size, None))
    t.cuda.synchronize()
    assert int(st.item()) == 0
    return out.cpu().numpy()[:size].tobytes()


class CountingLib:
    """the library with vga_hca_encode_device counted"""

    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if name != "vga_hca_encode_device":
            return f

        def counted(*a):
            self.calls += 1
            return f(*a)
        return counted


@pytest.mark.parametrize("code", [None, 0xCC55463930DBE1AB], ids=["plain", "keyed"])
def test_write_files_groups_looping_files(code, monkeypatch):
    key = crihca.CriHcaKey(code) if code is not None else None
    shapes = [(1, 5000, None), (1, 23000, None)] + [(1,) + (c[0], c[1:]) for c in lc.LOOP_CASES]
    shapes += [(2, 9000, (1024, 9000)), (2, 6000, None), (2, 20000, (14641, 15000)), (2, 4096, (4000, 4096)), (6, 5000, (0, 5000))]
    files, infos = [], []
    for k, (nch, n, loop) in enumerate(shapes):
        f = crihca.Pcm16Format(list(po.synth_generate(nch, n, first_channel=3 * k)), 48000)
        if loop:
            f.Looping, f.LoopStart, f.LoopEnd = True, loop[0], loop[1]
        files.append(f)
        infos.append(lc.info_of(lc.params_of(nch, n, loop)))
    groups, singles = hca.plan_write_groups(infos, [f.SampleCount for f in files])
    # mono 8b and the stereo 14641 file read their tails; the six-channel file is alone in its class
    assert singles == [10, 13, 15] and [len(g) for g in groups] == [10, 3]
    counting = CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: counting)
    got = hca.write_files(files, hca.HcaConfiguration(EncryptionKey=key))
    monkeypatch.undo()
    assert counting.calls == len(singles)
    for k, (f, h) in enumerate(zip(files, infos)):
        assert got[k] == per_file_image(f, h, key), ("file", k, shapes[k])

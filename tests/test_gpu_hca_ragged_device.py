"""Device-resident ragged HCA batches (include/vgaudio_hip/hca_ragged.h): vga_hca_decode_device_v / vga_hca_encode_device_v on
packed frames and packed PCM.  Every stream must be what the oracle makes of it alone and what its own vga_hca_*_device call
makes of it, bit for bit; nothing outside a stream's own rows may change.  All buffers are larger than needed and full of
junk.  The header is outside the lists the older test files enumerate, so this file carries its own table (CASES) of which
test exercises which function; tests/test_hca_ragged_device_host.py holds that table to the header."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from test_gpu_device_streams import delay  # noqa: F401  (the calibrated GPU delay that makes a caller's stream busy)
from vgaudio_amd import _lib
from vgaudio_amd.crihca import RaggedHca

pytestmark = pytest.mark.gpu

# function of the header -> the tests below that call it
CASES = {
    "vga_hca_ragged_layout_for": ["test_layout_of_the_object_is_the_host_layout"],
    "vga_hca_ragged_create": ["test_decode_matches_oracle_and_own_call", "test_stats"],
    "vga_hca_ragged_destroy": ["test_decode_matches_oracle_and_own_call"],
    "vga_hca_ragged_streams": ["test_layout_of_the_object_is_the_host_layout"],
    "vga_hca_ragged_totals_of": ["test_layout_of_the_object_is_the_host_layout"],
    "vga_hca_ragged_offsets": ["test_layout_of_the_object_is_the_host_layout"],
    "vga_hca_decode_device_v": ["test_decode_matches_oracle_and_own_call", "test_bytes_do_not_depend_on_poison_or_run_length",
                                "test_round_trip_on_a_busy_stream_and_two_streams_at_once", "test_bad_sync_word_marks_its_stream_only",
                                "test_refused_layouts_launch_nothing"],
    "vga_hca_encode_device_v": ["test_encode_matches_oracle_and_own_call", "test_bytes_do_not_depend_on_poison_or_run_length",
                                "test_round_trip_on_a_busy_stream_and_two_streams_at_once", "test_looping_stream_is_refused_by_encode",
                                "test_refused_layouts_launch_nothing"],
}

SENTINEL = 0x7777
JUNK = 0xEE
EXTRA = 64


def torch():
    import torch as t
    return t


def L():
    return _lib.lib()


def up(a):
    return torch().from_numpy(np.ascontiguousarray(a)).cuda()


class Stream:
    """one stream of a class: params, PCM, and the oracle's frames and decode of them"""

    def __init__(self, nch, n, k, loop=None):
        self.params = po.hca_params(nch, n, looping=bool(loop), loop_start=loop[0] if loop else 0, loop_end=loop[1] if loop else 0)
        self.pcm = po.synth_generate(nch, n, first_channel=8 * k)
        rc, oi, frames = po.hca_encode(self.pcm, self.params)
        assert rc == 0
        self.oinfo, self.frames = oi, frames.reshape(-1)
        self.info = _lib.HcaInfoC()
        cp = _lib.HcaParamsC(*[getattr(self.params, f) for f, _ in po.HcaParams._fields_])
        _lib.check(L().vga_hca_encoder_initialize(C.byref(cp), C.byref(self.info)))
        assert all(getattr(self.info, f) == getattr(oi, f) for f, _ in po.HcaInfo._fields_)
        rc, want = po.hca_decode(oi, frames)
        assert rc == 0
        self.want = np.ascontiguousarray(want)                       # [nch, sample_count]


def samples_for(frames, rng):
    """a sample count that gives `frames` frames (a plain stream leads in with 128 samples)"""
    return frames * 1024 - 128 - int(rng.integers(0, 1024 if frames > 1 else 800))


def make_classes():
    rng = np.random.default_rng(20261017)
    mono = [500, 7 * 1024 - 128, 0]                                  # 1 frame, 7 frames exactly, no samples
    while len(mono) < 38:
        n = samples_for(int(rng.integers(1, 25)), rng)
        if n not in mono:
            mono.append(n)
    streams = [Stream(1, n, k) for k, n in enumerate(mono)]
    streams.insert(5, Stream(1, 20000, 90, loop=(3000, 15000)))
    streams.insert(21, Stream(1, 9000, 91, loop=(1024, 9000)))
    stereo = [Stream(2, samples_for(int(f), rng), 100 + k) for k, f in enumerate(rng.integers(2, 17, 12))]
    six = [Stream(6, samples_for(f, rng), 120 + k) for k, f in enumerate((5, 9, 12))]
    assert len(streams) == 40 and all(1 <= s.info.frame_count <= 24 for s in streams if not s.info.looping)
    assert [s.info.frame_count for s in six] == [5, 9, 12]
    return {"mono": streams, "stereo": stereo, "six": six}


@pytest.fixture(scope="module")
def classes():
    return make_classes()


def plain(streams):
    return [s for s in streams if not s.info.looping]


class Batch:
    """a ragged object over `streams` and junk-filled packed buffers on the device"""

    def __init__(self, streams):
        self.streams = streams
        self.r = RaggedHca([s.info for s in streams])
        self.t, self.fo, self.ro = self.r.totals, self.r.frame_offsets, self.r.pcm_row_offsets
        self.rows = [(s, c) for s in streams for c in range(s.info.channel_count)]

    def close(self):
        self.r.close()

    # host images of the two buffers: junk everywhere, then (optionally) the streams' own data
    def frames_image(self, fill=True, junk=None):
        rng = np.random.default_rng(7)
        img = rng.integers(0, 256, self.t.frame_bytes + EXTRA, dtype=np.uint8) if junk is None else np.full(self.t.frame_bytes + EXTRA, junk, np.uint8)
        if fill:
            for s, at in zip(self.streams, self.fo):
                img[at:at + s.frames.size] = s.frames
        return img

    def pcm_image(self, fill=True):
        img = np.full(self.t.pcm_samples + EXTRA, SENTINEL, np.int16)
        if fill:
            for (s, c), at in zip(self.rows, self.ro):
                img[at:at + s.info.sample_count] = s.pcm[c, :s.info.sample_count]
        return img

    def workspace(self):
        return torch().full((self.t.decode_workspace_bytes + EXTRA,), 0xCD, dtype=torch().uint8, device="cuda")

    def status(self):
        return torch().zeros(len(self.streams) + 1, dtype=torch().int32, device="cuda")

    def decode(self, frames_img=None, stream=None):
        frames = up(self.frames_image() if frames_img is None else frames_img)
        pcm, st = up(self.pcm_image(fill=False)), self.status()
        self.r.decode_device(frames, pcm, self.workspace(), st, stream=stream)
        return frames, pcm, st

    def encode(self, stream=None):
        pcm, frames, st = up(self.pcm_image()), up(self.frames_image(fill=False, junk=JUNK)), self.status()
        self.r.encode_device(pcm, frames, st, stream=stream)
        return pcm, frames, st

    def check_pcm(self, got, what, skip=()):
        """got: host image after a decode: every row the oracle's, everything else untouched"""
        own = np.zeros(got.size, bool)
        for i, ((s, c), at) in enumerate(zip(self.rows, self.ro)):
            n = s.info.sample_count
            own[at:at + n] = True
            if self.streams.index(s) not in skip:
                assert np.array_equal(got[at:at + n], s.want[c]), (what, "row", i, "samples", n)
        assert np.all(got[~own] == SENTINEL), (what, "wrote outside the streams' own rows")

    def check_frames(self, got, what):
        own = np.zeros(got.size, bool)
        for i, (s, at) in enumerate(zip(self.streams, self.fo)):
            own[at:at + s.frames.size] = True
            assert np.array_equal(got[at:at + s.frames.size], s.frames), (what, "stream", i, "frames", s.info.frame_count)
        assert np.all(got[~own] == JUNK), (what, "wrote outside the streams' own frames")


@contextlib.contextmanager
def batch_of(streams):
    b = Batch(streams)
    try:
        yield b
    finally:
        torch().cuda.synchronize()
        b.close()


def own_decode(s):
    """one vga_hca_decode_device call for the stream -> ([nch, n] PCM, status)"""
    h, t = s.info, torch()
    pitch = (h.frame_count * h.frame_size + 8 + 3) // 4 * 4
    frames = t.zeros(pitch, dtype=t.uint8, device="cuda")
    frames[:s.frames.size] = up(s.frames)
    n = max(h.sample_count, 1)
    pcm = t.full((h.channel_count, n), SENTINEL, dtype=t.int16, device="cuda")
    wsb = L().vga_hca_decode_workspace_bytes(C.byref(h), 1)
    ws, st = t.empty(max(wsb, 16), dtype=t.uint8, device="cuda"), t.zeros(1, dtype=t.int32, device="cuda")
    _lib.check(L().vga_hca_decode_device(C.byref(h), frames.data_ptr(), pitch, 1, pcm.data_ptr(), h.channel_count * n, n, ws.data_ptr(),
                                         wsb, st.data_ptr(), None))
    t.cuda.synchronize()
    return pcm.cpu().numpy()[:, :h.sample_count], int(st.item())


def own_encode(s):
    h, t = s.info, torch()
    n = max(h.sample_count, 1)
    pcm = t.zeros((h.channel_count, n), dtype=t.int16, device="cuda")
    if h.sample_count:
        pcm[:, :h.sample_count] = up(s.pcm[:, :h.sample_count])
    pitch = (h.frame_count * h.frame_size + 8 + 3) // 4 * 4
    frames, st = t.zeros(pitch, dtype=t.uint8, device="cuda"), t.zeros(1, dtype=t.int32, device="cuda")
    _lib.check(L().vga_hca_encode_device(pcm.data_ptr(), h.channel_count * n, n, 1, h.sample_count, C.byref(h), frames.data_ptr(), pitch,
                                         st.data_ptr(), None))
    t.cuda.synchronize()
    assert int(st.item()) == 0
    return frames.cpu().numpy()[:h.frame_count * h.frame_size]


# ---------------------------------------------------------------- decode
@pytest.mark.parametrize("name", ["mono", "stereo", "six"])
def test_decode_matches_oracle_and_own_call(classes, name):
    streams = classes[name]
    with batch_of(streams) as b:
        frames, pcm, st = b.decode()
        torch().cuda.synchronize()
        assert np.all(st.cpu().numpy() == 0)
        b.check_pcm(pcm.cpu().numpy(), name)
        assert np.array_equal(frames.cpu().numpy(), b.frames_image()), "d_frames is an input"
    for k, s in enumerate(streams):                                   # the oracle's PCM is also each stream's own call's
        got, status = own_decode(s)
        assert status == 0 and np.array_equal(got, s.want), (name, k)


# ---------------------------------------------------------------- encode
@pytest.mark.parametrize("name", ["mono", "stereo", "six"])
def test_encode_matches_oracle_and_own_call(classes, name):
    streams = plain(classes[name])
    with batch_of(streams) as b:
        pcm, frames, st = b.encode()
        torch().cuda.synchronize()
        assert np.all(st.cpu().numpy() == 0)
        b.check_frames(frames.cpu().numpy(), name)
        assert np.array_equal(pcm.cpu().numpy(), b.pcm_image()), "d_pcm is an input"
    for k, s in enumerate(streams):
        assert np.array_equal(own_encode(s), s.frames), (name, k)


def test_looping_stream_is_refused_by_encode(classes):
    with batch_of(classes["mono"]) as b:
        assert any(s.info.looping for s in b.streams)
        pcm, frames, st = up(b.pcm_image()), up(b.frames_image(fill=False, junk=JUNK)), b.status()
        with pytest.raises(_lib.InvalidOperationError):
            b.r.encode_device(pcm, frames, st)
        torch().cuda.synchronize()
        assert np.all(frames.cpu().numpy() == JUNK)
        _, pcm, st = b.decode()                                       # the object is still good for decoding
        torch().cuda.synchronize()
        b.check_pcm(pcm.cpu().numpy(), "after the refusal")


# ---------------------------------------------------------------- poison mode, frames per run
@pytest.mark.parametrize("mode", ["poison-a5", "poison-ff", "run-1", "run-3", "run-16"])
def test_bytes_do_not_depend_on_poison_or_run_length(classes, mode):
    kind, _, value = mode.partition("-")
    if kind == "poison":
        old = L().vga_testing_poison_allocations(int(value, 16))
    else:
        old = L().vga_testing_hca_frames_per_group_this_thread(int(value))
    try:
        for name, streams in classes.items():
            with batch_of(streams) as b:                              # (created under the mode: its tables are poisoned first)
                _, pcm, st = b.decode()
                torch().cuda.synchronize()
                assert np.all(st.cpu().numpy() == 0)
                b.check_pcm(pcm.cpu().numpy(), (mode, name))
            with batch_of(plain(streams)) as b:
                _, frames, st = b.encode()
                torch().cuda.synchronize()
                assert np.all(st.cpu().numpy() == 0)
                b.check_frames(frames.cpu().numpy(), (mode, name))
    finally:
        torch().cuda.synchronize()
        if kind == "poison":
            L().vga_testing_poison_allocations(old if old >= 0 else -1)
        else:
            L().vga_testing_hca_frames_per_group_this_thread(old)


# ---------------------------------------------------------------- a busy caller stream, two streams at once
def test_round_trip_on_a_busy_stream_and_two_streams_at_once(classes, delay):  # noqa: F811
    t = torch()
    cycles, ms = delay
    streams = plain(classes["stereo"])
    with batch_of(streams) as b:
        A, B = t.cuda.Stream(), t.cuda.Stream()
        out = {}
        for name, S, busy in (("warm", A, False), ("A", A, True), ("B", B, False)):
            with t.cuda.stream(S):
                pcm_in, frames = up(b.pcm_image()), up(b.frames_image(fill=False, junk=JUNK))
                pcm_out, ws, st = up(b.pcm_image(fill=False)), b.workspace(), b.status()
                if busy:
                    t.cuda._sleep(cycles)
            b.r.encode_device(pcm_in, frames, st, stream=S)          # encode, then decode what it wrote: no host synchronisation
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
            b.check_pcm(pcm_out.cpu().numpy(), name)
        assert t.equal(out["A"][0], out["B"][0]) and t.equal(out["A"][1], out["B"][1])


# ---------------------------------------------------------------- a bad frame marks its own stream
def test_bad_sync_word_marks_its_stream_only(classes):
    streams = classes["stereo"]
    k = max(range(len(streams)), key=lambda i: streams[i].info.frame_count)
    h = streams[k].info
    assert h.frame_count >= 3
    with batch_of(streams) as b:
        img = b.frames_image()
        at = b.fo[k] + (h.frame_count // 2) * h.frame_size
        img[at] ^= 0xFF                                               # the sync word's first byte, a middle frame
        _, pcm, st = b.decode(frames_img=img)                         # (the wrapper raises on a non-zero return value)
        torch().cuda.synchronize()
        status = st.cpu().numpy()
        assert status[k] & 1, "the stream's own word carries the sync-word bit"
        assert np.all(np.delete(status, k) == 0)
        b.check_pcm(pcm.cpu().numpy(), "bad sync word", skip=(k,))


# ---------------------------------------------------------------- the object's numbers
def test_layout_of_the_object_is_the_host_layout(classes):
    for name, streams in classes.items():
        fo, ro, tot = RaggedHca.layout([s.info for s in streams])
        with batch_of(streams) as b:
            assert b.r.streams == len(streams) == L().vga_hca_ragged_streams(b.r._h)
            assert np.array_equal(fo, b.fo) and np.array_equal(ro, b.ro)
            assert all(getattr(tot, f) == getattr(b.t, f) for f, _ in tot._fields_)


def test_stats(classes):
    for name, streams in classes.items():
        with batch_of(streams) as b:
            v = (C.c_longlong * 4)()
            assert L().vga_testing_hca_ragged_stats(b.r._h, v, 4) == 4
            own = sum(s.info.frame_count for s in streams)
            assert v[0] == own == b.t.total_frames
            assert v[1] <= (own + 63) // 64 * 64
            assert v[2] == v[3] > 0


# ---------------------------------------------------------------- refused layouts
def test_refused_layouts_launch_nothing(classes):
    t = torch()
    with batch_of(plain(classes["stereo"])) as b:
        frames = up(np.concatenate([b.frames_image(), np.zeros(16, np.uint8)]))
        pcm = up(np.concatenate([b.pcm_image(fill=False), np.full(16, SENTINEL, np.int16)]))
        ws, st = b.workspace(), b.status()
        h, need = b.r._h, b.t.decode_workspace_bytes
        dec, enc = L().vga_hca_decode_device_v, L().vga_hca_encode_device_v
        assert dec(h, frames.data_ptr() + 1, pcm.data_ptr(), ws.data_ptr(), need, st.data_ptr(), None) == _lib.VGA_ERR_ARGUMENT
        assert dec(h, frames.data_ptr(), pcm.data_ptr() + 8, ws.data_ptr(), need, st.data_ptr(), None) == _lib.VGA_ERR_ARGUMENT
        assert dec(h, frames.data_ptr(), pcm.data_ptr(), ws.data_ptr(), need - 1, st.data_ptr(), None) == _lib.VGA_ERR_ARGUMENT
        out = up(b.frames_image(fill=False, junk=JUNK))
        assert enc(h, pcm.data_ptr() + 8, out.data_ptr(), st.data_ptr(), None) == _lib.VGA_ERR_ARGUMENT
        assert enc(h, pcm.data_ptr(), out.data_ptr() + 2, st.data_ptr(), None) == _lib.VGA_ERR_ARGUMENT
        t.cuda.synchronize()
        assert np.all(pcm.cpu().numpy() == SENTINEL) and np.all(out.cpu().numpy() == JUNK)
        assert np.all(ws.cpu().numpy() == 0xCD) and np.all(st.cpu().numpy() == 0)

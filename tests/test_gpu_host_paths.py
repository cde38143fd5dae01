"""The host-pointer entry points (what a P/Invoke caller calls) on the paths the rest of the suite never takes at its sizes:
the transfer kernels (gather of direct uploads, scatter of direct and of staged downloads, on CU-masked streams), more than
one compute lane, and a step that fails in the middle of a pipelined call.  Every call gets row pointers the test places
itself -- at every byte offset mod 16, next to neighbours in the same pages or alone in page-aligned allocations, with guard
bytes all around -- and every assertion is byte equality with the C oracle, untouched guard bytes and untouched inputs."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from vgaudio_amd import _lib

pytestmark = pytest.mark.gpu

i16p, u8p, cip = _lib.i16p, _lib.u8p, C.POINTER(C.c_int)
FILL = 0xA5
REFUSED = "step refused by vga_testing_fail_step_this_thread"
CHUNK = 2                                                     # units per chunk under the pipeline hook
# the two pipeline shapes of a forced transfer: direct rows both ways (one feeder: the gather, the drainers: the scatter),
# and staged rows through 8 KB ring slots (the staged scatter); pieces of 4 KB, so that rows of a few KB take several
DIRECT = dict(transfer=2, pipeline=(1, 2, CHUNK, -1), piece=4096)
STAGED = dict(transfer=2, pipeline=(2, 2, CHUNK, 8192), piece=4096)
SHAPES = {"direct": DIRECT, "staged": STAGED}


def L():
    return _lib.lib()


@contextlib.contextmanager
def hooks(transfer=0, pipeline=(0, 0, 0, 0), piece=0, lanes=0, tail=0, fail=(0, 0)):
    lib = L()
    lib.vga_testing_host_transfer_this_thread(transfer)
    lib.vga_testing_host_pipeline_this_thread(*pipeline)
    lib.vga_testing_host_transfer_piece_bytes_this_thread(piece)
    lib.vga_testing_host_compute_lanes_this_thread(lanes)
    lib.vga_testing_host_pipeline_tail_this_thread(tail)
    lib.vga_testing_fail_step_this_thread(*fail)
    try:
        yield
    finally:
        lib.vga_testing_host_transfer_this_thread(0)
        lib.vga_testing_host_pipeline_this_thread(0, 0, 0, 0)
        lib.vga_testing_host_transfer_piece_bytes_this_thread(0)
        lib.vga_testing_host_compute_lanes_this_thread(0)
        lib.vga_testing_host_pipeline_tail_this_thread(0)
        lib.vga_testing_fail_step_this_thread(0, 0)


@contextlib.contextmanager
def progress():
    seen = []
    fn = _lib.PROGRESS_FN(lambda _user, done, total: seen.append((done, total)))
    _lib.check(L().vga_set_progress_callback(C.cast(fn, C.c_void_p), None))
    try:
        yield seen
    finally:
        L().vga_set_progress_callback(None, None)


class Rows:
    """Rows of nbytes[i] bytes placed by the test.  Most share one buffer, `gap` guard bytes apart (neighbours share pages),
    row i at address = mods[i] (mod 16); every own-th row lies alone at the start of a page-aligned allocation.  Every byte
    that is not a row's is a guard byte (FILL)."""

    def __init__(self, nbytes, mods, own=4, gap=40):
        self.nbytes = [int(b) for b in nbytes]
        total = sum(self.nbytes) + (gap + 16) * (len(self.nbytes) + 2)
        self.parents = [np.full(total, FILL, np.uint8)]
        self.where = []
        pos = gap
        shared = 0
        for i, nb in enumerate(self.nbytes):
            if own and i % own == own - 1:
                a = np.full(nb + 2 * 4096 + gap, FILL, np.uint8)
                self.parents.append(a)
                self.where.append((len(self.parents) - 1, (-a.ctypes.data) % 4096))
            else:
                pos += (mods[shared % len(mods)] - (self.parents[0].ctypes.data + pos)) % 16
                shared += 1
                self.where.append((0, pos))
                pos += nb + gap
        assert pos + gap <= total

    def row(self, i, dtype=np.uint8):
        p, off = self.where[i]
        return self.parents[p][off:off + self.nbytes[i]].view(dtype)

    def ptrs(self, t):
        return (t * len(self.nbytes))(*[C.cast(C.c_void_p(self.parents[p].ctypes.data + off), t) for p, off in self.where])

    def snapshot(self):
        return [a.copy() for a in self.parents]

    def unchanged(self, snap):
        return all(np.array_equal(a, b) for a, b in zip(self.parents, snap))

    def guards_intact(self):
        for k, a in enumerate(self.parents):
            mask = np.ones(a.size, bool)
            for (p, off), nb in zip(self.where, self.nbytes):
                if p == k:
                    mask[off:off + nb] = False
            if not np.all(a[mask] == FILL):
                return False
        return True

    def clear(self):
        for i in range(len(self.nbytes)):
            self.row(i)[:] = FILL


def in_rows(arrays, mods, own=4):
    """input rows holding `arrays` (int16 rows at even offsets only)"""
    r = Rows([a.nbytes for a in arrays], mods, own)
    for i, a in enumerate(arrays):
        r.row(i, a.dtype)[:] = a
    return r


EVEN = list(range(0, 16, 2))
ALL = list(range(16))


def pcm_rows(lens, first=0):
    return [po.synth_generate(1, n, first_channel=first + c)[0].copy() if n else np.zeros(0, np.int16) for c, n in enumerate(lens)]


class Case:
    """One host-pointer call: inputs and outputs in placed rows, the oracle's expected outputs, extra host arrays with a
    guard tail.  call() returns the library's status code; check() asserts the whole picture."""
    units = 0

    def setup(self, ins, out_sizes, out_mods, expected, out_dtype):
        self.ins = ins
        self.snap = ins.snapshot()
        self.outs = Rows(out_sizes, out_mods)
        self.expected = expected
        self.out_dtype = out_dtype
        self.extra = []                                       # (array, valid length, expected or None)

    def host(self, n, dtype, fill, want=None):
        a = np.full(n + 8, fill, dtype)
        self.extra.append((a, n, fill, want))
        return a

    def clear(self):
        self.outs.clear()
        for a, n, fill, _ in self.extra:
            a[:] = fill

    def check(self, what=""):
        for i, want in enumerate(self.expected):
            got = self.outs.row(i, self.out_dtype)
            assert np.array_equal(got, want), (what, type(self).__name__, "row", i, int(np.argmax(got != want)) if got.size == want.size else (got.size, want.size))
        assert self.outs.guards_intact(), (what, type(self).__name__, "an output guard byte changed")
        assert self.ins.unchanged(self.snap), (what, type(self).__name__, "the call wrote to its input")
        for a, n, fill, want in self.extra:
            assert np.all(a[n:] == fill), (what, type(self).__name__, "wrote past a host array")
            if want is not None:
                assert np.array_equal(a[:n], want), (what, type(self).__name__, "host array")

    def run(self, what=""):
        self.clear()
        _lib.check(self.call())
        self.check(what)


# ---------------------------------------------------------------- GC-ADPCM
class GcEncode(Case):
    def __init__(self, nch=9, n=14 * 600 + 3, first=0):
        self.units, self.n = nch, n
        pcm = po.synth_generate(nch, n, first_channel=first)
        wc, wa = po.gc_encode_batch(pcm, threads=8)
        self.setup(in_rows(list(pcm), EVEN), [wa.shape[1]] * nch, ALL, list(wa), np.uint8)
        self.coefs = self.host(nch * 16, np.int16, 0x5A5A, wc.reshape(-1))

    def call(self):
        return L().vga_gcadpcm_encode_batch(self.ins.ptrs(i16p), self.units, self.n, 0, 0, self.coefs.ctypes.data_as(i16p),
                                            self.outs.ptrs(u8p))


class GcDecode(Case):
    def __init__(self, nch=9, n=14 * 600 + 3):
        self.units, self.n = nch, n
        pcm = po.synth_generate(nch, n, first_channel=100)
        wc, wa = po.gc_encode_batch(pcm, threads=8)
        self.coefs_in = np.ascontiguousarray(wc.reshape(-1))
        self.setup(in_rows(list(wa), ALL), [2 * n] * nch, EVEN, list(po.gc_decode_batch(wa, wc, n, threads=8)), np.int16)

    def call(self):
        return L().vga_gcadpcm_decode_batch(self.ins.ptrs(u8p), self.coefs_in.ctypes.data_as(i16p), self.units, self.n, None, None,
                                            self.outs.ptrs(i16p))


def samples_for_bytes(b):
    """a GC-ADPCM sample count whose byte count is b (b % 8 != 1: a frame's bytes are a header and 1..7 bytes of nibbles)"""
    q, p = divmod(b, 8)
    if p == 0:
        q, p = q - 1, 8
    assert p >= 2, b
    n = 14 * q + min(2 * p - 2, 13)
    assert po.gc_sample_count_to_byte_count(n) == b, (b, n)
    return n


RAGGED_LENS = [3000, 0, 14 * 300 + 1, 1, 14 * 600, 5000, 0, 9000, 14 * 292 + 13, 7777, 2048]


class GcEncodeV(Case):
    def __init__(self, lens=RAGGED_LENS, coefs_only=False, in_mods=EVEN, out_mods=ALL, own=4):
        self.units, self.coefs_only = len(lens), coefs_only
        self.counts = np.asarray(lens, np.int32)
        pcm = pcm_rows(lens, first=40)
        want_c = [po.gc_calculate_coefficients(p) for p in pcm]
        want_a = [po.gc_encode(p, c) for p, c in zip(pcm, want_c)]
        ins = in_rows(pcm, in_mods, own)
        if coefs_only:
            self.setup(ins, [], ALL, [], np.uint8)
        else:
            self.setup(ins, [a.size for a in want_a], out_mods, want_a, np.uint8)
        self.coefs = self.host(self.units * 16, np.int16, 0x5A5A, np.concatenate(want_c))

    def call(self):
        if self.coefs_only:
            return L().vga_gcadpcm_calculate_coefficients_batch_v(self.ins.ptrs(i16p), self.counts.ctypes.data_as(cip), self.units,
                                                                  self.coefs.ctypes.data_as(i16p))
        return L().vga_gcadpcm_encode_batch_v(self.ins.ptrs(i16p), self.counts.ctypes.data_as(cip), self.units, None, None,
                                              self.coefs.ctypes.data_as(i16p), self.outs.ptrs(u8p))


class GcDecodeV(Case):
    def __init__(self, lens=RAGGED_LENS, in_mods=ALL, out_mods=EVEN, own=4):
        self.units = len(lens)
        self.counts = np.asarray(lens, np.int32)
        pcm = pcm_rows(lens, first=70)
        coefs = [po.gc_calculate_coefficients(p) for p in pcm]
        adpcm = [po.gc_encode(p, c) for p, c in zip(pcm, coefs)]
        self.coefs_in = np.ascontiguousarray(np.concatenate(coefs))
        want = [po.gc_decode(a, c, n) for a, c, n in zip(adpcm, coefs, lens)]
        self.setup(in_rows(adpcm, in_mods, own), [2 * n for n in lens], out_mods, want, np.int16)

    def call(self):
        return L().vga_gcadpcm_decode_batch_v(self.ins.ptrs(u8p), self.coefs_in.ctypes.data_as(i16p), self.counts.ctypes.data_as(cip),
                                              self.units, None, None, self.outs.ptrs(i16p))


# ---------------------------------------------------------------- ADX
def adx_params():
    p = _lib.AdxParams()
    L().vga_adx_default_params(C.byref(p))
    return p


class AdxEncode(Case):
    def __init__(self, nch=7, n=32 * 200 + 13):
        self.units, self.n, self.p = nch, n, adx_params()
        pcm = po.synth_generate(nch, n, first_channel=200)
        want, hist = po.adx_encode_batch(pcm, po.adx_params(), threads=8)
        self.setup(in_rows(list(pcm), EVEN), [want.shape[1]] * nch, ALL, list(want), np.uint8)
        self.hist = self.host(nch, np.int16, 0x3C3C, hist)

    def call(self):
        return L().vga_adx_encode_batch(self.ins.ptrs(i16p), self.units, self.n, C.byref(self.p), self.outs.ptrs(u8p),
                                        self.hist.ctypes.data_as(i16p))


class AdxDecode(Case):
    def __init__(self, nch=7, n=32 * 200 + 13):
        self.units, self.n, self.p = nch, n, adx_params()
        pcm = po.synth_generate(nch, n, first_channel=300)
        enc, _ = po.adx_encode_batch(pcm, po.adx_params(), threads=8)
        self.nbytes = enc.shape[1]
        self.setup(in_rows(list(enc), ALL), [2 * n] * nch, EVEN, list(po.adx_decode_batch(enc, n, po.adx_params(), threads=8)), np.int16)

    def call(self):
        return L().vga_adx_decode_batch(self.ins.ptrs(u8p), self.nbytes, self.units, self.n, C.byref(self.p), self.outs.ptrs(i16p))


ADX_LENS = [3000, 31, 32 * 150, 5000, 64, 9000, 4100, 7777, 1, 2048]


class AdxEncodeV(Case):
    def __init__(self, lens=ADX_LENS):
        self.units = len(lens)
        self.counts = np.asarray(lens, np.int32)
        self.params = (_lib.AdxParams * self.units)(*[adx_params() for _ in lens])
        pcm = pcm_rows(lens, first=400)
        want = [po.adx_encode(p, po.adx_params()) for p in pcm]
        self.setup(in_rows(pcm, EVEN), [w.size for w in want], ALL, want, np.uint8)
        self.hist = self.host(self.units, np.int16, 0x3C3C)

    def call(self):
        return L().vga_adx_encode_batch_v(self.ins.ptrs(i16p), self.counts.ctypes.data_as(cip), self.units, self.params,
                                          self.outs.ptrs(u8p), self.hist.ctypes.data_as(i16p))


class AdxDecodeV(Case):
    def __init__(self, lens=ADX_LENS[:4] + [0] + ADX_LENS[4:]):
        self.units = len(lens)
        self.counts = np.asarray(lens, np.int32)
        self.params = (_lib.AdxParams * self.units)(*[adx_params() for _ in lens])
        pcm = pcm_rows(lens, first=500)
        enc = [po.adx_encode(p, po.adx_params()) if n else np.zeros(0, np.uint8) for p, n in zip(pcm, lens)]
        self.alens = np.asarray([e.size for e in enc], np.int32)
        want = [po.adx_decode(e, n, po.adx_params()) for e, n in zip(enc, lens)]
        self.setup(in_rows(enc, ALL), [2 * n for n in lens], EVEN, want, np.int16)

    def call(self):
        return L().vga_adx_decode_batch_v(self.ins.ptrs(u8p), self.alens.ctypes.data_as(cip), self.units, self.counts.ctypes.data_as(cip),
                                          self.params, self.outs.ptrs(i16p))


# ---------------------------------------------------------------- HCA
def hca_info(nch, n):
    cp = _lib.HcaParamsC(2, 0, 0, nch, 48000, n, 0, 0, 0)
    info = _lib.HcaInfoC()
    _lib.check(L().vga_hca_encoder_initialize(C.byref(cp), C.byref(info)))
    return cp, info


class HcaEncode(Case):
    def __init__(self, ns=7, nch=2, n=6000):
        self.units = ns
        self.cp, self.info = hca_info(nch, n)
        pcm = np.stack([po.synth_generate(nch, n, first_channel=600 + nch * s) for s in range(ns)])
        rc, _, want = po.hca_encode_batch(pcm, po.hca_params(nch, n), threads=8)
        assert rc == 0
        self.setup(in_rows([pcm[s, c] for s in range(ns) for c in range(nch)], EVEN), [want.shape[1]] * ns, ALL, list(want), np.uint8)

    def call(self):
        info = _lib.HcaInfoC()
        return L().vga_hca_encode_batch(self.ins.ptrs(i16p), self.units, C.byref(self.cp), C.byref(info), self.outs.ptrs(u8p))


class HcaDecode(Case):
    def __init__(self, ns=7, nch=2, n=6000):
        self.units = ns
        self.cp, self.info = hca_info(nch, n)
        pcm = np.stack([po.synth_generate(nch, n, first_channel=700 + nch * s) for s in range(ns)])
        rc, pinfo, frames = po.hca_encode_batch(pcm, po.hca_params(nch, n), threads=8)
        rc2, want = po.hca_decode_batch(pinfo, frames, threads=8)
        assert rc == 0 and rc2 == 0
        self.setup(in_rows(list(frames), ALL), [2 * n] * (ns * nch), EVEN, [want[s, c] for s in range(ns) for c in range(nch)], np.int16)

    def call(self):
        return L().vga_hca_decode_batch(C.byref(self.info), self.ins.ptrs(u8p), self.units, self.outs.ptrs(i16p))


# vga_hca_decode_batch_v decodes the streams of one HcaInfo per call, in the order of their first appearance: the last call
# here has three streams (two chunks)
HCA_STREAMS = [(2, 1024), (2, 9000), (1, 100), (2, 3000), (1, 6000), (2, 3000), (1, 6000), (2, 3000), (1, 6000)]


class HcaEncodeV(Case):
    def __init__(self, streams=HCA_STREAMS):
        self.units = len(streams)
        self.cps = (_lib.HcaParamsC * self.units)(*[hca_info(c, n)[0] for c, n in streams])
        rows, want = [], []
        for s, (nch, n) in enumerate(streams):
            pcm = po.synth_generate(nch, n, first_channel=800 + 2 * s)
            rc, _, frames = po.hca_encode(pcm, po.hca_params(nch, n))
            assert rc == 0
            rows += list(pcm)
            want.append(frames.reshape(-1))
        self.setup(in_rows(rows, EVEN), [w.size for w in want], ALL, want, np.uint8)

    def call(self):
        infos = (_lib.HcaInfoC * self.units)()
        return L().vga_hca_encode_batch_v(self.ins.ptrs(i16p), self.units, self.cps, infos, self.outs.ptrs(u8p))


class HcaDecodeV(Case):
    def __init__(self, streams=HCA_STREAMS):
        self.units = len(streams)
        self.infos = (_lib.HcaInfoC * self.units)(*[hca_info(c, n)[1] for c, n in streams])
        frames_rows, want, sizes = [], [], []
        for s, (nch, n) in enumerate(streams):
            pcm = po.synth_generate(nch, n, first_channel=900 + 2 * s)
            rc, pinfo, frames = po.hca_encode(pcm, po.hca_params(nch, n))
            rc2, dec = po.hca_decode(pinfo, frames)
            assert rc == 0 and rc2 == 0
            frames_rows.append(frames.reshape(-1))
            want += list(dec)
            sizes += [2 * n] * nch
        self.setup(in_rows(frames_rows, ALL), sizes, EVEN, want, np.int16)

    def call(self):
        return L().vga_hca_decode_batch_v(self.infos, self.ins.ptrs(u8p), self.units, self.outs.ptrs(i16p))


CASES = {
    "gc_encode_batch": GcEncode, "gc_decode_batch": GcDecode, "gc_encode_batch_v": GcEncodeV,
    "gc_coefs_batch_v": lambda: GcEncodeV(coefs_only=True), "gc_decode_batch_v": GcDecodeV,
    "adx_encode_batch": AdxEncode, "adx_decode_batch": AdxDecode, "adx_encode_batch_v": AdxEncodeV, "adx_decode_batch_v": AdxDecodeV,
    "hca_encode_batch": HcaEncode, "hca_decode_batch": HcaDecode, "hca_encode_batch_v": HcaEncodeV, "hca_decode_batch_v": HcaDecodeV,
}
_built = {}


def case(name):
    if name not in _built:
        _built[name] = CASES[name]()
    return _built[name]


# ---------------------------------------------------------------- 1. every entry point with the transfer kernels forced on
@pytest.mark.parametrize("name", list(CASES))
def test_transfer_kernels_forced_on_give_the_oracles_bytes(name):
    c = case(name)
    c.run("default path")
    for shape, kw in SHAPES.items():
        with hooks(**kw):
            c.run(shape)
        stats = (C.c_double * 32)()
        L().vga_testing_last_pipeline_stats(stats, 32)
        assert stats[15] >= min(2, -(-c.units // CHUNK)), (shape, "chunks", stats[15])


# ---------------------------------------------------------------- 2. row placement grid
def _grid_lengths():
    """byte counts of GC-ADPCM rows: every residue mod 16 a GC-ADPCM row can have (8q + 1 cannot occur), and 4096 k - 1, 4096 k
    around the transfer kernels' pieces; a few empty rows"""
    sizes = [b for b in range(32, 48) if b % 8 != 1] + [b for b in range(4096 + 16, 4096 + 32) if b % 8 != 1]
    sizes += [4095, 4096, 2 * 4096 - 1, 2 * 4096, 3 * 4096 - 1, 3 * 4096, 4096 + 2, 2 * 4096 + 2]
    return [samples_for_bytes(b) for b in sizes] + [0, 0]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_rows_at_every_offset_and_length_residue_through_the_transfer_kernels(shape):
    lens = _grid_lengths()
    rng = np.random.default_rng(5)
    lens = [lens[i] for i in rng.permutation(len(lens))]
    # byte rows at every offset 0..15 (output of the encode, input of the decode), int16 rows at the even offsets; PCM rows of
    # 2 n bytes also land on 8190 / 8192 / 8194 ... around the pieces
    enc = GcEncodeV(lens, in_mods=[(3 * i) % 16 & ~1 for i in range(16)], out_mods=ALL, own=5)
    dec = GcDecodeV(lens, in_mods=[(5 * i + 3) % 16 for i in range(16)], out_mods=EVEN, own=3)
    with hooks(**SHAPES[shape]):
        enc.run(shape)
        dec.run(shape)


def test_int16_rows_around_whole_pieces():
    """PCM rows of 4096 k - 2, 4096 k and 4096 k + 2 bytes (plus odd residues of their sample counts) at every even offset"""
    lens = [2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 6145, 1, 2, 3, 4, 5, 6, 7, 8]
    for shape in SHAPES:
        with hooks(**SHAPES[shape]):
            GcEncodeV(lens, in_mods=EVEN, out_mods=[(7 * i) % 16 for i in range(16)], own=6).run(shape)
            GcDecodeV(lens, in_mods=[(7 * i) % 16 for i in range(16)], out_mods=[14, 2, 0, 8, 6, 4, 12, 10], own=6).run(shape)


# ---------------------------------------------------------------- 3. compute lanes 1..4
LANE_TRANSFER = {"transfer off": dict(transfer=1), "transfer forced": dict(transfer=2, piece=4096)}


@pytest.mark.parametrize("transfer", list(LANE_TRANSFER))
@pytest.mark.parametrize("lanes", [1, 2, 3, 4])
def test_gc_encoders_on_every_lane_count(lanes, transfer):
    kw = LANE_TRANSFER[transfer]
    big = GcEncode(nch=17, n=14 * 200 + 9, first=1000)                  # 9 chunks of 2: chunk k on lane k % lanes
    ragged = GcEncodeV(RAGGED_LENS + RAGGED_LENS[::-1][:6])             # 17 channels, 9 chunks
    coefs_only = GcEncodeV(RAGGED_LENS, coefs_only=True)
    with hooks(pipeline=(1, 2, CHUNK, -1), lanes=lanes, **kw):
        big.run((lanes, transfer))
        ragged.run((lanes, transfer))
        coefs_only.run((lanes, transfer))
        stats = (C.c_double * 32)()
        L().vga_testing_last_pipeline_stats(stats, 32)
        assert stats[15] >= 6
    # one channel (one chunk, one lane), and two channels in one chunk that the tail hook splits in two (both lanes)
    one, two = GcEncode(nch=1, n=14 * 900 + 5, first=1100), GcEncode(nch=2, n=14 * 900 + 5, first=1200)
    with hooks(lanes=lanes, **kw):
        one.run((lanes, transfer, "one channel"))
    with hooks(lanes=lanes, tail=1, **kw):
        two.run((lanes, transfer, "two channels, split chunk"))
        stats = (C.c_double * 32)()
        L().vga_testing_last_pipeline_stats(stats, 32)
        assert stats[15] == 2


@pytest.mark.parametrize("transfer", list(LANE_TRANSFER))
@pytest.mark.parametrize("name", ["adx_encode_batch", "adx_decode_batch_v", "hca_encode_batch", "hca_decode_batch", "hca_encode_batch_v",
                                  "gc_decode_batch", "gc_decode_batch_v"])
def test_stateless_entry_points_on_two_lanes(name, transfer):
    """ADX, HCA and the GC decoders keep nothing per lane: two lanes give the same bytes"""
    with hooks(pipeline=(1, 2, CHUNK, -1), lanes=2, **LANE_TRANSFER[transfer]):
        case(name).run((2, transfer))


# ---------------------------------------------------------------- 4. injected failures
def _refuse_and_retry(c, kw, kind, nth, what):
    c.clear()
    with progress() as seen, hooks(fail=(kind, nth), **kw):
        rc = c.call()
    assert rc == _lib.VGA_ERR_DEVICE, (what, rc)
    assert L().vga_last_error().decode() == REFUSED, what
    assert all(total == c.units for _, total in seen), (what, seen)
    assert all(done <= c.units for done, _ in seen), (what, seen)
    assert c.ins.unchanged(c.snap), (what, "the failed call wrote to its input")
    # the same call with the same caller buffers
    with hooks(**kw):
        c.run(what + " retried")


@pytest.mark.parametrize("transfer", list(LANE_TRANSFER))
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("name", ["gc_encode_batch", "gc_encode_batch_v", "adx_encode_batch_v", "hca_encode_batch"])
def test_a_refused_step_fails_the_call_and_the_retry_gives_the_oracles_bytes(name, lanes, transfer):
    c = case(name)
    kw = dict(pipeline=(1, 2, CHUNK, -1), lanes=lanes, **LANE_TRANSFER[transfer])
    with hooks(**kw):
        c.run("before")
        stats = (C.c_double * 32)()
        L().vga_testing_last_pipeline_stats(stats, 32)
    chunks = int(stats[15])
    assert chunks >= 3, chunks
    for nth in sorted({1, (chunks + 1) // 2, chunks}):
        _refuse_and_retry(c, kw, _lib.VGA_TESTING_STEP_CHUNK_COMPUTE, nth, f"chunk {nth} of {chunks}")
    if kw["transfer"] == 2:
        for nth in (1, 2):
            _refuse_and_retry(c, kw, _lib.VGA_TESTING_STEP_TRANSFER, nth, f"transfer launch {nth}")

"""The *_device entry points on a busy caller stream (include/vgaudio_hip.h: "*_device entry points run on the caller's
stream and never synchronise it").

One table, ROWS, holds a row per device entry point of the header.  Each row builds its inputs, calls the entry point and
compares every output byte with an independent reference (oracle/pyoracle.py or the restatements in tests/*_ref.py).
A row runs on a fresh non-blocking stream S:

  1. warm-up: one call on S with the same shape, then synchronise (code-object loads and pool growth may block);
  2. poison: on S, every input buffer the call reads is filled with one junk byte, every output buffer with another;
  3. delay: on S, a bounded GPU sleep of about 250 ms (calibrated once per session against torch.cuda.Event timing);
  4. late inputs: on S, the real inputs are copied over the poisoned ones;
  5. the call, with S as its stream, timed on the host;
  6. right after it returns, S must still be busy and the call must have taken under half the delay (HOST_RESULT rows
     return a host value and must synchronise: they skip this step);
  7. S.synchronize(): the call returned VGA_OK, status words are 0 and every output byte equals the reference.

Work the library puts on another stream runs during the delay and reads the poisoned inputs (wrong output); a host-side
wait turns step 6 into a failure.  The delay ends on its own, so a broken library cannot hang the test.
A second test runs two calls of one entry point at once on two streams (the second overtakes the first while it waits
behind its delay): both outputs must be right.  The ragged `_v` forms share one vga_gcadpcm_ragged handle there.
"""
import contextlib
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry points that return a host value and so must synchronise the caller's stream (the header says so)
HOST_RESULT = {"vga_adx_find_key_device", "vga_hca_find_key_device", "vga_hca_byte_position_counts_device"}

TARGET_MS = 250.0
MIN_MS = 150.0
MAX_MS = 2000.0
POISON_IN, POISON_OUT = 0xA5, 0x5A


def header_device_entry_points():
    """every vga_*_device / vga_*_device_v function the public header declares, vga_set_device aside"""
    text = open(os.path.join(ROOT, "include", "vgaudio_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(vga_\w+_device(?:_v)?)\s*\(", text))
    return names - {"vga_set_device"}


def header_synchronising_entry_points():
    """the device entry points whose declaration comment says they synchronise the caller's stream"""
    text = open(os.path.join(ROOT, "include", "vgaudio_hip.h")).read()
    out = set()
    for comment, decl in re.findall(r"/\*((?:(?!\*/).)*)\*/\s*\n(?:\w[^;]*?)\b(vga_\w+_device)\s*\(", text, flags=re.S):
        if re.search(r"synchronises the caller's stream", comment):
            out.add(decl)
    return out


# ====================================================================== helpers (GPU only below this line)
def _torch():
    import torch
    return torch


def _L():
    from vgaudio_amd import _lib
    return _lib.lib()


def _up(a):
    """host array -> contiguous device tensor (same dtype)"""
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


JUNK = "junk"
_PAD = {"fill": 0}                                          # what _rows / _packed put where no row lies, unless told otherwise


@contextlib.contextmanager
def pad_fill(fill):
    """inside the block, rows are padded with `fill` instead of zeros (test_gpu_dirty_memory.py: JUNK)"""
    old, _PAD["fill"] = _PAD["fill"], fill
    try:
        yield
    finally:
        _PAD["fill"] = old


def _filled(shape, dtype, fill):
    """an array of `fill`; JUNK: seeded random values over the whole range of dtype"""
    if fill is None:
        fill = _PAD["fill"]
    if isinstance(fill, str):
        assert fill == JUNK
        info = np.iinfo(dtype)
        return np.random.default_rng(0xD1).integers(info.min, info.max + 1, shape).astype(dtype)
    return np.full(shape, fill, dtype=dtype)


def _rows(rows, pitch, dtype, fill=None):
    """list of 1-D arrays -> [len(rows), pitch] host array, padded with `fill` (default 0; see pad_fill)"""
    out = _filled((len(rows), pitch), dtype, fill)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def _pitch(n, m=16, extra=16):
    """a pitch past the minimum: a multiple of m (16 by default) that is not a multiple of 256"""
    p = (n + m - 1) // m * m + extra
    while p % 256 == 0:
        p += m
    return p


class Case:
    """One call's buffers: `inputs` are the device buffers the call reads (real contents in `real`), `outputs` the
    buffers it writes; `call(stream)` returns the status code; `check()` compares the outputs with the reference."""

    def __init__(self, inputs, outputs, call, check):
        torch = _torch()
        self.inputs = [t for t in inputs if t is not None]
        self.real = [t.clone() for t in self.inputs]
        self.outputs = [t for t in outputs if t is not None]
        self.call = call
        self.check = check
        for t in self.inputs + self.outputs:
            assert t.is_contiguous()
        torch.cuda.synchronize()

    def poison(self):
        for t in self.inputs:
            t.view(-1).view(_torch().uint8).fill_(POISON_IN)
        for t in self.outputs:
            t.view(-1).view(_torch().uint8).fill_(POISON_OUT)

    def load(self):
        """the real inputs, padding included: what _rows put behind the rows (zeros or junk) is restored with them"""
        for t, r in zip(self.inputs, self.real):
            t.copy_(r)

    inplace_cols = None                                     # rows that work in place: the columns of inputs[0] the call rewrites

    def inputs_unchanged(self):
        """every input byte the call may not write still holds what load() put there"""
        for i, (t, r) in enumerate(zip(self.inputs, self.real)):
            if i == 0 and self.inplace_cols is not None:
                t, r = t[:, self.inplace_cols:], r[:, self.inplace_cols:]
            if not bool((t == r).all()):
                return False
        return True


def _ok(rc):
    from vgaudio_amd import _lib
    assert rc == 0, f"rc {rc}: {_lib.lib().vga_last_error().decode(errors='replace')}"


def _eq(got_t, want, what):
    got = got_t.cpu().numpy()
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}")


def _zero_status(t):
    assert int(t.cpu().numpy().view(np.int32).reshape(-1)[0]) == 0, "device status word is not 0"


# ====================================================================== rows: GC-ADPCM
def _gc_data(k, nch=67, n=14 * 150 + 5):
    from oracle import pyoracle as po
    pcm = po.synth_generate(nch, n, first_channel=100 * k)
    coefs, adpcm = po.gc_encode_batch(pcm)
    return pcm, coefs, adpcm


def row_gc_coefs(k, shared, n=14 * 150 + 5):
    L = _L()
    torch = _torch()
    pcm, coefs, _ = _gc_data(k, n=n)
    nch = pcm.shape[0]
    d_pcm = _up(_rows(pcm, _pitch(n, 8), np.int16))
    ws_bytes = L.vga_gcadpcm_coefs_workspace_bytes(nch, n)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
    out = torch.empty((nch, 16), dtype=torch.int16, device="cuda")
    return Case([d_pcm], [out],
                lambda s: L.vga_gcadpcm_coefs_device(d_pcm.data_ptr(), d_pcm.shape[1], nch, n, out.data_ptr(), ws.data_ptr(),
                                                     ws.numel(), s),
                lambda: _eq(out, coefs, "coefs"))


def row_gc_encode(k, shared, n=14 * 150 + 5):
    L = _L()
    torch = _torch()
    pcm, coefs, adpcm = _gc_data(k, n=n)
    nch, nb = adpcm.shape
    d_pcm = _up(_rows(pcm, _pitch(n, 8), np.int16))
    d_coefs = _up(coefs)
    out = torch.empty((nch, _pitch(nb)), dtype=torch.uint8, device="cuda")
    return Case([d_pcm, d_coefs], [out],
                lambda s: L.vga_gcadpcm_encode_device(d_pcm.data_ptr(), d_pcm.shape[1], nch, n, d_coefs.data_ptr(), None, None,
                                                      out.data_ptr(), out.shape[1], s),
                lambda: _eq(out[:, :nb], adpcm, "adpcm"))


def row_gc_encode_seams(k, shared):
    """long enough for 12 time pieces of 64 frames or more: the seam chain and the persistent queue run on S"""
    return row_gc_encode(k, shared, n=14 * 64 * 14 + 9)


def row_gc_decode(k, shared):
    from oracle import pyoracle as po
    L = _L()
    torch = _torch()
    n = 14 * 150 + 5
    pcm, coefs, adpcm = _gc_data(k, n=n)
    nch, nb = adpcm.shape
    want = po.gc_decode_batch(adpcm, coefs, n)
    d_adpcm = _up(_rows(adpcm, _pitch(nb), np.uint8))
    d_coefs = _up(coefs)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.empty((nch, _pitch(n, 8)), dtype=torch.int16, device="cuda")
    return Case([d_adpcm, d_coefs, status], [out],
                lambda s: L.vga_gcadpcm_decode_device(d_adpcm.data_ptr(), d_adpcm.shape[1], d_coefs.data_ptr(), nch, n, None, None,
                                                      out.data_ptr(), out.shape[1], status.data_ptr(), s),
                lambda: (_eq(out[:, :n], want, "pcm"), _zero_status(status)))


RAGGED_COUNTS = [1000, 14 * 300 + 3, 37, 20001, 5, 14 * 64, 3333, 14]


def _ragged(shared):
    from vgaudio_amd.device import GcRaggedBatch
    if "ragged" not in shared:
        shared["ragged"] = GcRaggedBatch(RAGGED_COUNTS, "cuda")
    return shared["ragged"]


def _ragged_data(k):
    from oracle import pyoracle as po
    chans = [po.synth_generate(1, n, first_channel=50 * k + c)[0] for c, n in enumerate(RAGGED_COUNTS)]
    coefs = np.stack([po.gc_calculate_coefficients(a) for a in chans])
    adpcm = [po.gc_encode(a, coefs[c]) for c, a in enumerate(chans)]
    return chans, coefs, adpcm


def _packed(r, rows, offsets, total, dtype, fill=None):
    host = _filled(total, dtype, fill)
    for o, a in zip(offsets, rows):
        host[int(o):int(o) + len(a)] = a
    return host


def _packed_eq(flat, rows, offsets, what):
    host = flat.cpu().numpy()
    for c, (o, a) in enumerate(zip(offsets, rows)):
        got = host[int(o):int(o) + len(a)]
        assert np.array_equal(got, a), f"{what}: channel {c} differs"


def row_gc_coefs_v(k, shared):
    L = _L()
    torch = _torch()
    r = _ragged(shared)
    chans, coefs, _ = _ragged_data(k)
    d_pcm = _up(_packed(r, chans, r.pcm_offsets, r.pcm_samples, np.int16))
    ws = torch.empty(max(r.workspace_bytes, 16), dtype=torch.uint8, device="cuda")
    out = torch.empty((r.nch, 16), dtype=torch.int16, device="cuda")
    return Case([d_pcm], [out],
                lambda s: L.vga_gcadpcm_coefs_device_v(r.handle, d_pcm.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), s),
                lambda: _eq(out, coefs, "coefs"))


def row_gc_encode_v(k, shared):
    L = _L()
    torch = _torch()
    r = _ragged(shared)
    chans, coefs, adpcm = _ragged_data(k)
    d_pcm = _up(_packed(r, chans, r.pcm_offsets, r.pcm_samples, np.int16))
    d_coefs = _up(coefs)
    out = torch.empty(r.adpcm_bytes, dtype=torch.uint8, device="cuda")
    return Case([d_pcm, d_coefs], [out],
                lambda s: L.vga_gcadpcm_encode_device_v(r.handle, d_pcm.data_ptr(), d_coefs.data_ptr(), None, None, out.data_ptr(), s),
                lambda: _packed_eq(out, adpcm, r.adpcm_offsets, "adpcm"))


def row_gc_decode_v(k, shared):
    from oracle import pyoracle as po
    L = _L()
    torch = _torch()
    r = _ragged(shared)
    chans, coefs, adpcm = _ragged_data(k)
    want = [po.gc_decode(a, coefs[c], RAGGED_COUNTS[c]) for c, a in enumerate(adpcm)]
    d_adpcm = _up(_packed(r, adpcm, r.adpcm_offsets, r.adpcm_bytes, np.uint8))
    d_coefs = _up(coefs)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.empty(r.pcm_samples, dtype=torch.int16, device="cuda")
    return Case([d_adpcm, d_coefs, status], [out],
                lambda s: L.vga_gcadpcm_decode_device_v(r.handle, d_adpcm.data_ptr(), d_coefs.data_ptr(), None, None, out.data_ptr(),
                                                        status.data_ptr(), s),
                lambda: (_packed_eq(out, want, r.pcm_offsets, "pcm"), _zero_status(status)))


def row_gc_build_channels(k, shared):
    from oracle import pyoracle as po
    from vgaudio_amd import _lib
    L = _L()
    torch = _torch()
    n = 20000
    pcm, coefs, adpcm = _gc_data(k, nch=67, n=n)
    nch, nb = adpcm.shape
    op = po.gc_channel_params(n, True, 1234, n, 700, 14 * 64)
    p = _lib.GcChannelParamsC(n, 1, 1234, n, 700, 14 * 64)
    want = [po.gc_build_channel(adpcm[c], coefs[c], op) for c in range(nch)]
    lay = want[0][1]
    na, ns, ne = po.gc_sample_count_to_byte_count(lay.sample_count_aligned), lay.sample_count_aligned, lay.seek_table_entries
    d_adpcm = _up(_rows(adpcm, _pitch(nb), np.uint8))
    d_coefs = _up(coefs)
    a_out = torch.empty((nch, _pitch(na)), dtype=torch.uint8, device="cuda")
    p_out = torch.empty((nch, _pitch(ns, 8)), dtype=torch.int16, device="cuda")
    s_out = torch.empty((nch, _pitch(2 * ne, 8)), dtype=torch.int16, device="cuda")
    c_out = torch.empty((nch, 3), dtype=torch.int16, device="cuda")
    wsb = L.vga_gcadpcm_build_channels_workspace_bytes(nch, C.byref(p))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")

    def check():
        for c in range(nch):
            rc, _, wa, wp, wsk, wctx = want[c]
            assert rc == 0
            _eq(a_out[c, :na], wa, f"adpcm {c}")
            _eq(p_out[c, :ns], wp, f"pcm {c}")
            _eq(s_out[c, :2 * ne], wsk, f"seek {c}")
            _eq(c_out[c], wctx, f"loop context {c}")
    return Case([d_adpcm, d_coefs], [a_out, p_out, s_out, c_out],
                lambda s: L.vga_gcadpcm_build_channels_device(d_adpcm.data_ptr(), d_adpcm.shape[1], d_coefs.data_ptr(), nch, C.byref(p),
                                                              a_out.data_ptr(), a_out.shape[1], p_out.data_ptr(), p_out.shape[1],
                                                              s_out.data_ptr(), s_out.shape[1], c_out.data_ptr(), ws.data_ptr(), wsb, s),
                check)


# ====================================================================== rows: GC-ADPCM containers
def _rand_gc_rows(k, nch, nb, nfiles=1):
    rng = np.random.default_rng(1000 + k)
    adpcm = rng.integers(0, 256, (nfiles * nch, nb)).astype(np.uint8)
    adpcm[:, 0] &= 0x7F                                         # a predictor below 8 in every first header
    coefs = rng.integers(-2000, 2000, (nfiles * nch, 16)).astype(np.int16)
    start = rng.integers(-3000, 3000, (nfiles * nch, 3)).astype(np.int16)
    loop = rng.integers(-3000, 3000, (nfiles * nch, 3)).astype(np.int16)
    start[:, 0] &= 0x7F
    loop[:, 0] &= 0x7F
    return rng, adpcm, coefs, start, loop


def row_dsp_write(k, shared):
    from oracle import pyoracle as po
    from vgaudio_amd import _lib
    L = _L()
    torch = _torch()
    nch, n = 3, 14 * 0x800 * 2 + 9
    nb = po.gc_sample_count_to_byte_count(n)
    _, adpcm, coefs, start, loop = _rand_gc_rows(k, nch, nb)
    gain = np.arange(nch, dtype=np.int16) * 7 + k
    op = po.dsp_params(32000, n, samples_per_interleave=14 * 0x800)
    rc, want = po.dsp_write(list(adpcm), coefs, op, gain=gain, start_context=start, loop_context=loop)
    assert rc == 0
    p = _lib.DspParamsC(32000, n, 0, 0, 0, 14 * 0x800, 1, 1)
    d_adpcm, d_coefs, d_gain, d_start, d_loop = (_up(_rows(adpcm, _pitch(nb), np.uint8)), _up(coefs), _up(gain), _up(start), _up(loop))
    out = torch.empty(len(want) + 40, dtype=torch.uint8, device="cuda")
    return Case([d_adpcm, d_coefs, d_gain, d_start, d_loop], [out],
                lambda s: L.vga_dsp_write_device(d_adpcm.data_ptr(), d_adpcm.shape[1], nb, d_coefs.data_ptr(), d_gain.data_ptr(),
                                                 d_start.data_ptr(), d_loop.data_ptr(), nch, C.byref(p), out.data_ptr(), s),
                lambda: _eq(out[:len(want)], want, "DSP image"))


def _images_on_device(images):
    """equally long byte images -> ([nfiles, pitch] uint8 tensor, pitch)"""
    size = len(images[0])
    fp = _pitch(size)
    return _up(_rows([np.frombuffer(bytes(i), np.uint8) for i in images], fp, np.uint8)), fp


def row_dsp_read(k, shared):
    from oracle import pyoracle as po
    from vgaudio_amd import _lib
    L = _L()
    torch = _torch()
    nch, n, nf = 3, 14 * 0x800 * 2 + 9, 3
    nb = po.gc_sample_count_to_byte_count(n)
    _, adpcm, coefs, start, loop = _rand_gc_rows(k, nch, nb, nf)
    op = po.dsp_params(32000, n, samples_per_interleave=14 * 0x800)
    images = []
    for f in range(nf):
        rc, img = po.dsp_write(list(adpcm[f * nch:f * nch + nch]), coefs[f * nch:f * nch + nch], op)
        assert rc == 0
        images.append(img)
    want = [po.dsp_read(img)[-1] for img in images]
    info = _lib.DspInfoC()
    _ok(L.vga_dsp_parse(images[0].ctypes.data_as(_lib.u8p), len(images[0]), C.byref(info)))
    files, fp = _images_on_device(images)
    ab = info.adpcm_bytes
    out = torch.empty((nf * nch, _pitch(ab)), dtype=torch.uint8, device="cuda")
    return Case([files], [out],
                lambda s: L.vga_dsp_read_device(C.byref(info), files.data_ptr(), fp, nf, out.data_ptr(), out.shape[1], s),
                lambda: [_eq(out[f * nch + c, :ab], want[f][c][:ab], f"file {f} channel {c}") for f in range(nf) for c in range(nch)])


def _nw_params(n):
    from vgaudio_amd import _lib
    p = _lib.NwParamsC()
    p.target, p.sample_rate, p.sample_count, p.endianness = 2, 44100, n, -1
    p.samples_per_interleave, p.samples_per_seek_table_entry = 14 * 64, 14 * 32
    lay = _lib.NwLayoutC()
    _ok(_L().vga_nwstm_layout_for(C.byref(p), 2, C.byref(lay)))
    return p, lay


def _nw_images(k, nch, nf, n):
    import nwstm_ref as ref
    p, lay = _nw_params(n)
    nb, ne = lay.channel_adpcm_bytes, lay.channel_seek_entries
    rng, adpcm, coefs, start, loop = _rand_gc_rows(k, nch, nb, nf)
    seek = rng.integers(-30000, 30000, (nf * nch, 2 * ne)).astype(np.int16)
    images = []
    for f in range(nf):
        rows = range(f * nch, f * nch + nch)
        images.append(ref.build_image(2, 44100, nch, [adpcm[r].tobytes() for r in rows], [coefs[r].tolist() for r in rows],
                                      [0] * nch, [[int(adpcm[r, 0]), 0, 0] for r in rows], [loop[r].tolist() for r in rows],
                                      [seek[r].tolist() for r in rows], lay.looping, lay.loop_start, lay.loop_end,
                                      lay.sample_count, spi=lay.samples_per_interleave, spe=lay.samples_per_seek_table_entry,
                                      version=lay.version))
    return p, lay, adpcm, coefs, loop, seek, images


def row_nwstm_write(k, shared):
    L = _L()
    torch = _torch()
    nch, nf, n = 2, 3, 14 * 64 * 5 + 11
    p, lay, adpcm, coefs, loop, seek, images = _nw_images(k, nch, nf, n)
    nb, ne = lay.channel_adpcm_bytes, lay.channel_seek_entries
    d_adpcm, d_coefs, d_loop = _up(_rows(adpcm, _pitch(nb), np.uint8)), _up(coefs), _up(loop)
    d_seek = _up(_rows(seek, _pitch(2 * ne, 8), np.int16))
    fp = _pitch(lay.file_size)
    out = torch.empty((nf, fp), dtype=torch.uint8, device="cuda")
    return Case([d_adpcm, d_coefs, d_loop, d_seek], [out],
                lambda s: L.vga_nwstm_write_device(C.byref(p), nch, nf, None, d_adpcm.data_ptr(), d_adpcm.shape[1], nb,
                                                   d_coefs.data_ptr(), None, None, d_loop.data_ptr(), d_seek.data_ptr(),
                                                   d_seek.shape[1], ne, out.data_ptr(), fp, s),
                lambda: [_eq(out[f, :lay.file_size], np.frombuffer(images[f], np.uint8), f"image {f}") for f in range(nf)])


def row_nwstm_read(k, shared):
    from vgaudio_amd import _lib
    L = _L()
    torch = _torch()
    nch, nf, n = 2, 3, 14 * 64 * 5 + 11
    p, lay, adpcm, coefs, loop, seek, images = _nw_images(k, nch, nf, n)
    info = _lib.NwInfoC()
    one = np.frombuffer(images[0], np.uint8).copy()
    _ok(L.vga_nwstm_parse(one.ctypes.data_as(_lib.u8p), len(one), C.byref(info)))
    files, fp = _images_on_device(images)
    ab = info.adpcm_bytes
    out = torch.empty((nf * nch, _pitch(ab)), dtype=torch.uint8, device="cuda")
    return Case([files], [out],
                lambda s: L.vga_nwstm_read_device(C.byref(info), files.data_ptr(), fp, nf, out.data_ptr(), out.shape[1], s),
                lambda: _eq(out[:, :ab], adpcm[:, :ab], "rows"))


def _hps_images(k, nch, nf, n):
    import gc_containers_ref as ref
    nb = ref.bytes_of(n)
    rng, adpcm, coefs, start, _ = _rand_gc_rows(k, nch, nb, nf)
    gain = rng.integers(-100, 100, nf * nch).astype(np.int16)
    pcm = rng.integers(-30000, 30000, (nf * nch, n)).astype(np.int16)
    images = []
    for f in range(nf):
        rows = range(f * nch, f * nch + nch)
        images.append(ref.hps_image(32000, [adpcm[r].tobytes() for r in rows], [coefs[r].tolist() for r in rows],
                                    [int(gain[r]) for r in rows], [start[r].tolist() for r in rows], [pcm[r] for r in rows],
                                    False, 0, 0, n))
    return nb, adpcm, coefs, gain, start, pcm, images


def row_hps_write(k, shared):
    from vgaudio_amd import _lib
    L = _L()
    torch = _torch()
    nch, nf, n = 2, 3, 0x10000 + 14 * 300 + 3         # two blocks per file
    nb, adpcm, coefs, gain, start, pcm, images = _hps_images(k, nch, nf, n)
    p = _lib.HpsParamsC(32000, n, 0, 0, 0)
    d_adpcm, d_coefs, d_gain, d_start = _up(_rows(adpcm, _pitch(nb), np.uint8)), _up(coefs), _up(gain), _up(start)
    d_pcm = _up(_rows(pcm, _pitch(n, 8), np.int16))
    size = len(images[0])
    fp = _pitch(size)
    out = torch.empty((nf, fp), dtype=torch.uint8, device="cuda")
    return Case([d_adpcm, d_coefs, d_gain, d_start, d_pcm], [out],
                lambda s: L.vga_hps_write_device(C.byref(p), nch, nf, d_adpcm.data_ptr(), d_adpcm.shape[1], nb, d_coefs.data_ptr(),
                                                 d_gain.data_ptr(), d_start.data_ptr(), d_pcm.data_ptr(), d_pcm.shape[1], n,
                                                 out.data_ptr(), fp, s),
                lambda: [_eq(out[f, :size], np.frombuffer(bytes(images[f]), np.uint8), f"image {f}") for f in range(nf)])


def row_hps_read(k, shared):
    from vgaudio_amd.hps import parse
    L = _L()
    torch = _torch()
    nch, nf, n = 2, 3, 0x10000 + 14 * 300 + 3
    nb, adpcm, coefs, gain, start, pcm, images = _hps_images(k, nch, nf, n)
    info, blocks = parse(bytes(images[0]))
    files, fp = _images_on_device(images)
    ab = info.adpcm_bytes
    out = torch.empty((nf * nch, _pitch(ab)), dtype=torch.uint8, device="cuda")
    return Case([files], [out],
                lambda s: L.vga_hps_read_device(C.byref(info), blocks, files.data_ptr(), fp, nf, out.data_ptr(), out.shape[1], s),
                lambda: _eq(out[:, :ab], adpcm[:, :ab], "rows"))


def _idsp_images(k, nch, nf, n):
    import gc_containers_ref as ref
    nb = ref.bytes_of(n)
    rng, adpcm, coefs, start, loop = _rand_gc_rows(k, nch, nb, nf)
    images = []
    for f in range(nf):
        rows = range(f * nch, f * nch + nch)
        images.append(ref.idsp_image(32000, [adpcm[r].tobytes() for r in rows], [coefs[r].tolist() for r in rows], [0] * nch,
                                     [start[r].tolist() for r in rows], [loop[r].tolist() for r in rows], False, 0, 0, n, 0x10, True))
    return nb, adpcm, coefs, start, loop, images


def row_idsp_write(k, shared):
    from vgaudio_amd import _lib
    L = _L()
    torch = _torch()
    nch, nf, n = 3, 3, 14 * 700 + 5
    nb, adpcm, coefs, start, loop, images = _idsp_images(k, nch, nf, n)
    p = _lib.IdspParamsC(32000, n, 0, 0, 0, 0x10, 1)
    d_adpcm, d_coefs, d_start, d_loop = _up(_rows(adpcm, _pitch(nb), np.uint8)), _up(coefs), _up(start), _up(loop)
    size = len(images[0])
    fp = _pitch(size)
    out = torch.empty((nf, fp), dtype=torch.uint8, device="cuda")
    return Case([d_adpcm, d_coefs, d_start, d_loop], [out],
                lambda s: L.vga_idsp_write_device(C.byref(p), nch, nf, d_adpcm.data_ptr(), d_adpcm.shape[1], nb, d_coefs.data_ptr(),
                                                  None, d_start.data_ptr(), d_loop.data_ptr(), out.data_ptr(), fp, s),
                lambda: [_eq(out[f, :size], np.frombuffer(bytes(images[f]), np.uint8), f"image {f}") for f in range(nf)])


def row_idsp_read(k, shared):
    from vgaudio_amd.idsp import parse
    L = _L()
    torch = _torch()
    nch, nf, n = 3, 3, 14 * 700 + 5
    nb, adpcm, coefs, start, loop, images = _idsp_images(k, nch, nf, n)
    info = parse(bytes(images[0]))
    files, fp = _images_on_device(images)
    ab = info.adpcm_bytes
    out = torch.empty((nf * nch, _pitch(ab)), dtype=torch.uint8, device="cuda")
    return Case([files], [out],
                lambda s: L.vga_idsp_read_device(C.byref(info), files.data_ptr(), fp, nf, out.data_ptr(), out.shape[1], s),
                lambda: _eq(out[:, :ab], adpcm[:, :ab], "rows"))


def row_genh_read(k, shared):
    import gc_containers_ref as ref
    from vgaudio_amd.genh import parse
    L = _L()
    torch = _torch()
    nch, nf, n = 2, 4, 14 * 900 + 3
    nb = ref.bytes_of(n)
    _, adpcm, coefs, _, _ = _rand_gc_rows(k, nch, nb, nf)
    images = [ref.genh_image(48000, [adpcm[f * nch + c].tobytes() for c in range(nch)],
                             [coefs[f * nch + c].tolist() for c in range(nch)], 0x40, -1, n, 0) for f in range(nf)]
    info = parse(bytes(images[0]))
    files, fp = _images_on_device(images)
    ab = info.adpcm_bytes
    out = torch.empty((nf * nch, _pitch(ab)), dtype=torch.uint8, device="cuda")
    return Case([files], [out],
                lambda s: L.vga_genh_read_device(C.byref(info), files.data_ptr(), fp, nf, out.data_ptr(), out.shape[1], s),
                lambda: _eq(out[:, :ab], adpcm[:, :ab], "rows"))


# ====================================================================== rows: ADX
def _adx_params(**kw):
    from oracle import pyoracle as po
    from vgaudio_amd import _lib
    p = _lib.AdxParams()
    _L().vga_adx_default_params(C.byref(p))
    for key, v in kw.items():
        setattr(p, key, v)
    return p, po.adx_params(**kw)


def row_adx_encode(k, shared, n=32 * 300 + 7, padding=0):
    from oracle import pyoracle as po
    L = _L()
    torch = _torch()
    nch = 67
    pcm = po.synth_generate(nch, n, first_channel=300 + 100 * k)
    p, op = _adx_params(padding=padding)
    want, whist = po.adx_encode_batch(pcm, op)
    nb = want.shape[1]
    d_pcm = _up(_rows(pcm, _pitch(n, 8), np.int16))
    out = torch.empty((nch, _pitch(nb)), dtype=torch.uint8, device="cuda")
    hist = torch.empty(nch + 8, dtype=torch.int16, device="cuda")
    return Case([d_pcm], [out, hist],
                lambda s: L.vga_adx_encode_device(d_pcm.data_ptr(), d_pcm.shape[1], nch, n, C.byref(p), out.data_ptr(), out.shape[1],
                                                  hist.data_ptr(), s),
                lambda: (_eq(out[:, :nb], want, "adx"), _eq(hist[:nch], whist, "history")))


def row_adx_encode_seams(k, shared):
    return row_adx_encode(k, shared, n=32 * 64 * 14 + 5, padding=13)


def row_adx_decode(k, shared, n=32 * 300 + 7, padding=0):
    from oracle import pyoracle as po
    L = _L()
    torch = _torch()
    nch = 67
    pcm = po.synth_generate(nch, n, first_channel=600 + 100 * k)
    p, op = _adx_params(padding=padding)
    adx, _ = po.adx_encode_batch(pcm, op)
    want = po.adx_decode_batch(adx, n, op)
    nb = adx.shape[1]
    d_adx = _up(_rows(adx, _pitch(nb), np.uint8))
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.empty((nch, _pitch(n, 8)), dtype=torch.int16, device="cuda")
    return Case([d_adx, status], [out],
                lambda s: L.vga_adx_decode_device(d_adx.data_ptr(), d_adx.shape[1], nb, nch, n, C.byref(p), out.data_ptr(), out.shape[1],
                                                  status.data_ptr(), s),
                lambda: (_eq(out[:, :n], want, "pcm"), _zero_status(status)))


def row_adx_decode_seams(k, shared):
    return row_adx_decode(k, shared, n=32 * 64 * 14 + 5, padding=13)


def _adx_files(k, nch, nf, n):
    from oracle import pyoracle as po
    pcm = po.synth_generate(nf * nch, n, first_channel=900 + 100 * k)
    _, op = _adx_params()
    audio, hist = po.adx_encode_batch(pcm, op)
    fp = po.adxfile_params(48000, n)
    images = []
    for f in range(nf):
        rc, img = po.adxfile_write(list(audio[f * nch:f * nch + nch]), hist[f * nch:f * nch + nch], fp)
        assert rc == 0
        images.append(img)
    return audio, hist, images


def row_adx_write(k, shared):
    from vgaudio_amd import _lib
    L = _L()
    torch = _torch()
    nch, n = 5, 32 * 500 + 3
    audio, hist, images = _adx_files(k, nch, 1, n)
    nb = audio.shape[1]
    p = _lib.AdxFileParamsC(48000, n, 0, 0, 0, 0, 18, 4, 3, 500, 0, 1)
    d_audio, d_hist = _up(_rows(audio, _pitch(nb), np.uint8)), _up(hist)
    out = torch.empty(len(images[0]) + 40, dtype=torch.uint8, device="cuda")
    return Case([d_audio, d_hist], [out],
                lambda s: L.vga_adx_write_device(d_audio.data_ptr(), d_audio.shape[1], nb, d_hist.data_ptr(), nch, C.byref(p),
                                                 out.data_ptr(), s),
                lambda: _eq(out[:len(images[0])], images[0], "ADX image"))


def row_adx_read(k, shared):
    from oracle import pyoracle as po
    from vgaudio_amd import _lib
    L = _L()
    torch = _torch()
    nch, nf, n = 3, 3, 32 * 500 + 3
    audio, hist, images = _adx_files(k, nch, nf, n)
    info = _lib.AdxFileInfoC()
    _ok(L.vga_adx_parse(images[0].ctypes.data_as(_lib.u8p), len(images[0]), C.byref(info)))
    want = [po.adxfile_read(img)[3] for img in images]
    files, fp = _images_on_device(images)
    ab = info.audio_bytes
    out = torch.empty((nf * nch, _pitch(ab)), dtype=torch.uint8, device="cuda")
    return Case([files], [out],
                lambda s: L.vga_adx_read_device(C.byref(info), files.data_ptr(), fp, nf, out.data_ptr(), out.shape[1], s),
                lambda: [_eq(out[f * nch + c, :ab], want[f][c][:ab], f"file {f} channel {c}") for f in range(nf) for c in range(nch)])


# ====================================================================== rows: HCA
def _hca(nch, n, quality="High"):
    from oracle import pyoracle as po
    from vgaudio_amd import _lib
    q = po.HCA_QUALITY[quality]
    cfg = _lib.HcaParamsC(q, 0, 0, nch, 48000, n, 0, 0, 0)
    info = _lib.HcaInfoC()
    _ok(_L().vga_hca_encoder_initialize(C.byref(cfg), C.byref(info)))
    return info, po.hca_params(nch, n, quality=quality)


def _hca_frames(k, ns, nch, n, quality="High"):
    from oracle import pyoracle as po
    pcm = po.synth_generate(ns * nch, n, first_channel=1200 + 100 * k).reshape(ns, nch, n)
    info, op = _hca(nch, n, quality)
    rc, oinfo, frames = po.hca_encode_batch(pcm, op)
    assert rc == 0
    return pcm, info, oinfo, frames


def row_hca_encode(k, shared):
    L = _L()
    torch = _torch()
    ns, nch, n = 3, 2, 1024 * 9 + 100
    pcm, info, oinfo, want = _hca_frames(k, ns, nch, n)
    cp = _pitch(n, 8)
    d_pcm = _up(_rows(pcm.reshape(ns * nch, n), cp, np.int16))
    fb = want.shape[1]
    fp = _pitch(fb)
    out = torch.empty((ns, fp), dtype=torch.uint8, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    return Case([d_pcm, status], [out],
                lambda s: L.vga_hca_encode_device(d_pcm.data_ptr(), nch * cp, cp, ns, n, C.byref(info), out.data_ptr(), fp,
                                                  status.data_ptr(), s),
                lambda: (_eq(out[:, :fb], want, "frames"), _zero_status(status)))


def row_hca_decode(k, shared):
    from oracle import pyoracle as po
    L = _L()
    torch = _torch()
    ns, nch, n = 3, 2, 1024 * 9 + 100
    pcm, info, oinfo, frames = _hca_frames(k, ns, nch, n)
    rc, want = po.hca_decode_batch(oinfo, frames)
    assert rc == 0
    fb = frames.shape[1]
    d_frames = _up(_rows(frames, _pitch(fb + 8), np.uint8))
    ws_bytes = L.vga_hca_decode_workspace_bytes(C.byref(info), ns)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
    cp = _pitch(n, 8)
    out = torch.empty((ns, nch, cp), dtype=torch.int16, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    return Case([d_frames, status], [out],
                lambda s: L.vga_hca_decode_device(C.byref(info), d_frames.data_ptr(), d_frames.shape[1], ns, out.data_ptr(), nch * cp, cp,
                                                  ws.data_ptr(), ws_bytes, status.data_ptr(), s),
                lambda: (_eq(out[:, :, :n], want, "pcm"), _zero_status(status)))


def _hca_files(k, ns, nch, n):
    from oracle import pyoracle as po
    pcm, info, oinfo, frames = _hca_frames(k, ns, nch, n)
    images = []
    for s in range(ns):
        rc, img = po.hcafile_write(oinfo, frames[s])
        assert rc == 0
        images.append(img)
    return info, frames, images


def row_hca_write(k, shared):
    L = _L()
    torch = _torch()
    ns, nch, n = 3, 2, 1024 * 9 + 100
    info, frames, images = _hca_files(k, ns, nch, n)
    fb = frames.shape[1]
    d_frames = _up(_rows(frames, _pitch(fb), np.uint8))
    size = len(images[0])
    fp = _pitch(size)
    out = torch.empty((ns, fp), dtype=torch.uint8, device="cuda")
    return Case([d_frames], [out],
                lambda s: L.vga_hca_write_device(C.byref(info), d_frames.data_ptr(), d_frames.shape[1], ns, None, 1.0, 0, 0,
                                                 out.data_ptr(), fp, s),
                lambda: [_eq(out[f, :size], images[f], f"image {f}") for f in range(ns)])


def row_hca_read(k, shared):
    from vgaudio_amd import _lib
    L = _L()
    torch = _torch()
    ns, nch, n = 3, 2, 1024 * 9 + 100
    info, frames, images = _hca_files(k, ns, nch, n)
    fi = _lib.HcaFileInfoC()
    _ok(L.vga_hca_parse(images[0].ctypes.data_as(_lib.u8p), len(images[0]), C.byref(fi)))
    files, fp = _images_on_device(images)
    fb = frames.shape[1]
    out = torch.empty((ns, _pitch(fb + 8)), dtype=torch.uint8, device="cuda")
    bad = torch.empty(ns + 4, dtype=torch.int32, device="cuda")
    want = np.concatenate([frames, np.zeros((ns, 8), np.uint8)], axis=1)
    return Case([files], [out, bad],
                lambda s: L.vga_hca_read_device(C.byref(fi), files.data_ptr(), fp, ns, out.data_ptr(), out.shape[1], bad.data_ptr(), s),
                lambda: (_eq(out[:, :fb + 8], want, "frames"), _eq(bad[:ns], np.zeros(ns, np.int32), "bad CRC counts")))


# ====================================================================== rows: synth, WAVE
def row_synth(k, shared):
    from oracle import pyoracle as po
    from vgaudio_amd import synth
    L = _L()
    torch = _torch()
    nch, n, first = 67, 5000 + 3, 40 + 100 * k
    want = po.synth_generate(nch, n, first_channel=first)
    params = _up(np.array([synth.channel_params(first + c) for c in range(nch)], dtype=np.uint32).view(np.int32))
    out = torch.empty((nch, _pitch(n, 8)), dtype=torch.int16, device="cuda")
    return Case([params], [out],
                lambda s: L.vga_synth_pcm16_device(out.data_ptr(), out.shape[1], nch, n, first, params.data_ptr(), s),
                lambda: _eq(out[:, :n], want, "pcm"))


def row_wave_deinterleave(k, shared):
    L = _L()
    torch = _torch()
    nch, n = 6, 30000 + 7
    rng = np.random.default_rng(50 + k)
    pcm = rng.integers(-32768, 32768, (nch, n)).astype(np.int16)
    data = _up(np.ascontiguousarray(pcm.T).view(np.uint8).reshape(-1))
    out = torch.empty((nch, _pitch(n, 8)), dtype=torch.int16, device="cuda")
    return Case([data], [out],
                lambda s: L.vga_wave_deinterleave_pcm16_device(data.data_ptr(), n, nch, out.data_ptr(), out.shape[1], s),
                lambda: _eq(out[:, :n], pcm, "pcm"))


def row_wave_write(k, shared):
    from oracle import pyoracle as po
    from vgaudio_amd import _lib
    L = _L()
    torch = _torch()
    nch, n = 6, 30000 + 7
    rng = np.random.default_rng(60 + k)
    pcm = rng.integers(-32768, 32768, (nch, n)).astype(np.int16)
    rc, want = po.wave_write(list(pcm), 44100)
    assert rc == 0
    p = _lib.WaveParamsC(44100, n, 0, 0, 0)
    d_pcm = _up(_rows(pcm, _pitch(n, 8), np.int16))
    out = torch.empty(len(want) + 40, dtype=torch.uint8, device="cuda")
    return Case([d_pcm], [out],
                lambda s: L.vga_wave_write_pcm16_device(d_pcm.data_ptr(), d_pcm.shape[1], nch, C.byref(p), out.data_ptr(), s),
                lambda: _eq(out[:len(want)], want, "WAVE image"))


# ====================================================================== rows: encryption
def _adx_keys():
    from vgaudio_amd import _lib
    L = _L()
    keys = (_lib.AdxKeyC * 6)()
    for i, name in enumerate((b"GHM", b"GHMSC", b"karaage", b"mituba", b"morio", b"ranatus")):
        _ok(L.vga_adx_key_from_string(name, C.byref(keys[i])))
    return keys


def _okey(key):
    from oracle import pyoracle as po
    return po.AdxKey(key.seed, key.mult, key.inc)


def row_adx_crypt(k, shared):
    from oracle import pyoracle as po
    L = _L()
    torch = _torch()
    nch, frames = 67, 301
    rng = np.random.default_rng(70 + k)
    audio = rng.integers(0, 256, (nch, 18 * frames)).astype(np.uint8)
    key = _adx_keys()[2 + k]
    want = np.stack(po.adx_crypt(list(audio), _okey(key), 8))
    d = _up(_rows(audio, _pitch(18 * frames), np.uint8))
    case = Case([d], [],
                lambda s: L.vga_adx_crypt_device(d.data_ptr(), d.shape[1], 18 * frames, nch, C.byref(key), 8, 18, s),
                lambda: _eq(d[:, :18 * frames], want, "audio"))
    case.inplace_cols = 18 * frames
    return case


def row_adx_find_key(k, shared):
    from oracle import pyoracle as po
    L = _L()
    nch, n = 3, 32 * 800
    pcm = po.synth_generate(nch, n, first_channel=77 + k)
    _, op = _adx_params()
    audio, _ = po.adx_encode_batch(pcm, op)
    keys = _adx_keys()
    target = 4 - k
    enc = np.stack(po.adx_crypt(list(audio), _okey(keys[target]), 8))
    want = next(i for i in range(len(keys)) if po.adx_test_key(list(enc), _okey(keys[i]), 8))
    assert want == target
    nb = enc.shape[1]
    d = _up(_rows(enc, _pitch(nb), np.uint8))
    idx = C.c_int(-7)

    def check():
        assert idx.value == want
    return Case([d], [],
                lambda s: L.vga_adx_find_key_device(d.data_ptr(), d.shape[1], nb, nch, 8, 18, keys, len(keys), C.byref(idx), s),
                check)


def row_hca_crypt(k, shared):
    from oracle import pyoracle as po
    from vgaudio_amd import _lib
    L = _L()
    ns, fc, fs = 3, 37, 682
    rng = np.random.default_rng(80 + k)
    frames = rng.integers(0, 256, (ns, fc * fs)).astype(np.uint8)
    rc, dec, enc = po.hca_key_tables(56, 123456789 + k)
    want = np.stack([po.hca_crypt(frames[s], fs, enc) for s in range(ns)])
    d = _up(_rows(frames, _pitch(fc * fs), np.uint8))
    case = Case([d], [],
                lambda s: L.vga_hca_crypt_device(d.data_ptr(), d.shape[1], ns, fc, fs, enc.ctypes.data_as(_lib.u8p), s),
                lambda: _eq(d[:, :fc * fs], want, "frames"))
    case.inplace_cols = fc * fs
    return case


def row_hca_find_key(k, shared):
    from oracle import pyoracle as po
    from vgaudio_amd import _lib
    L = _L()
    nch, n = 2, 1024 * 14
    pcm, info, oinfo, frames = _hca_frames(k, 1, nch, n)
    rng = np.random.default_rng(90 + k)
    codes = [int(c) for c in rng.integers(1, 2 ** 56, 9)]
    tables = [po.hca_key_tables(56, c) for c in codes]
    true = 6 - k
    enc = po.hca_crypt(frames[0], info.frame_size, tables[true][2]).reshape(-1, info.frame_size)
    dtabs = np.ascontiguousarray(np.stack([t[1] for t in tables]))
    want = po.hca_find_key(oinfo, enc, dtabs)
    assert want == true
    d = _up(enc.reshape(-1))
    idx = C.c_int(-7)

    def check():
        assert idx.value == want
    return Case([d], [],
                lambda s: L.vga_hca_find_key_device(C.byref(info), d.data_ptr(), info.frame_count, dtabs.ctypes.data_as(_lib.u8p),
                                                    len(codes), C.byref(idx), s),
                check)


def row_hca_byte_position_counts(k, shared):
    from oracle import pyoracle as po
    L = _L()
    ns, fc, fs = 5, 37, 100
    rng = np.random.default_rng(100 + k)
    frames = rng.integers(0, 256, (ns, fc * fs)).astype(np.uint8)
    want = po.hca_byte_position_counts(frames, fs, 30)
    d = _up(_rows(frames, _pitch(fc * fs), np.uint8))
    counts = np.zeros((30, 256), dtype=np.uint32)

    def check():
        assert np.array_equal(counts, want)
    return Case([d], [],
                lambda s: L.vga_hca_byte_position_counts_device(d.data_ptr(), d.shape[1], ns, fc, fs, 30, counts.ctypes.data, s),
                check)


# ====================================================================== the table
# entry point -> row builder (k selects one of two independent data sets; `shared` is per test)
ROWS = {
    "vga_gcadpcm_coefs_device": row_gc_coefs,
    "vga_gcadpcm_encode_device": row_gc_encode,
    "vga_gcadpcm_decode_device": row_gc_decode,
    "vga_gcadpcm_coefs_device_v": row_gc_coefs_v,
    "vga_gcadpcm_encode_device_v": row_gc_encode_v,
    "vga_gcadpcm_decode_device_v": row_gc_decode_v,
    "vga_gcadpcm_build_channels_device": row_gc_build_channels,
    "vga_dsp_write_device": row_dsp_write,
    "vga_dsp_read_device": row_dsp_read,
    "vga_nwstm_write_device": row_nwstm_write,
    "vga_nwstm_read_device": row_nwstm_read,
    "vga_hps_write_device": row_hps_write,
    "vga_hps_read_device": row_hps_read,
    "vga_idsp_write_device": row_idsp_write,
    "vga_idsp_read_device": row_idsp_read,
    "vga_genh_read_device": row_genh_read,
    "vga_adx_encode_device": row_adx_encode,
    "vga_adx_decode_device": row_adx_decode,
    "vga_adx_write_device": row_adx_write,
    "vga_adx_read_device": row_adx_read,
    "vga_hca_encode_device": row_hca_encode,
    "vga_hca_decode_device": row_hca_decode,
    "vga_synth_pcm16_device": row_synth,
    "vga_hca_write_device": row_hca_write,
    "vga_hca_read_device": row_hca_read,
    "vga_wave_deinterleave_pcm16_device": row_wave_deinterleave,
    "vga_wave_write_pcm16_device": row_wave_write,
    "vga_adx_crypt_device": row_adx_crypt,
    "vga_adx_find_key_device": row_adx_find_key,
    "vga_hca_crypt_device": row_hca_crypt,
    "vga_hca_find_key_device": row_hca_find_key,
    "vga_hca_byte_position_counts_device": row_hca_byte_position_counts,
}

# the multi-launch paths: time pieces (vga_testing_gc_encoder_segments_this_thread) with every seam left open
# (vga_testing_force_open_seams_this_thread): seam chain, REPAIR launch, persistent queue and their memsets on S
SEAM_ROWS = {
    "vga_gcadpcm_encode_device": row_gc_encode_seams,
    "vga_adx_encode_device": row_adx_encode_seams,
    "vga_adx_decode_device": row_adx_decode_seams,
}

# entry points that take scratch or keep launch state: run two calls at once
CONCURRENT = ["vga_gcadpcm_coefs_device", "vga_gcadpcm_encode_device", "vga_gcadpcm_decode_device",
              "vga_gcadpcm_coefs_device_v", "vga_gcadpcm_encode_device_v", "vga_gcadpcm_decode_device_v",
              "vga_adx_encode_device", "vga_adx_decode_device", "vga_hca_encode_device", "vga_hca_decode_device",
              "vga_hps_write_device", "vga_hps_read_device"]


# ====================================================================== the CPU check: the table covers the header
def test_table_covers_every_device_entry_point():
    declared = header_device_entry_points()
    assert len(declared) >= 32
    assert set(ROWS) == declared, f"missing rows: {sorted(declared - set(ROWS))}, stale rows: {sorted(set(ROWS) - declared)}"
    assert set(SEAM_ROWS) <= set(ROWS) and set(CONCURRENT) <= set(ROWS)


def test_host_result_set_is_what_the_header_says_synchronises():
    assert header_synchronising_entry_points() == HOST_RESULT
    assert HOST_RESULT <= set(ROWS)


# ====================================================================== the GPU tests
@pytest.fixture(scope="module")
def delay():
    """(cycles, ms): a torch.cuda._sleep of about TARGET_MS, measured with events on a stream of its own"""
    torch = _torch()
    s = torch.cuda.Stream()

    def measure(cycles):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            a.record()
            torch.cuda._sleep(int(cycles))
            b.record()
        b.synchronize()
        return a.elapsed_time(b)

    measure(1000)
    cycles, ms = 1_000_000, 0.0
    for _ in range(6):                                      # grow the probe until it lasts a few milliseconds
        ms = measure(cycles)
        if ms >= 5.0:
            break
        cycles *= 8
    assert ms > 0.0, "torch.cuda._sleep took no measurable time"
    per_ms = cycles / ms
    cycles = int(min(TARGET_MS, MAX_MS * 0.8) * per_ms)
    ms = measure(cycles)
    if ms > MAX_MS:
        cycles = int(cycles * TARGET_MS / ms)
        ms = measure(cycles)
    assert MIN_MS <= ms <= MAX_MS, f"calibrated GPU delay is {ms:.1f} ms ({cycles} cycles): outside {MIN_MS}..{MAX_MS} ms"
    print(f"\n[device streams] delay calibration: {per_ms:.0f} cycles/ms, {cycles} cycles = {ms:.1f} ms")
    yield cycles, ms
    if HOST_TIMES:                                          # the margin the delay leaves (shown with -s)
        worst = max(HOST_TIMES, key=HOST_TIMES.get)
        print(f"\n[device streams] longest host call of a non-synchronising entry point: {HOST_TIMES[worst]:.2f} ms ({worst})")


HOST_TIMES = {}


def _run_on_busy_stream(name, case, S, delay):
    """steps 2-6 on S; returns the call's status code (S may still be running)"""
    torch = _torch()
    cycles, ms = delay
    with torch.cuda.stream(S):
        case.poison()
        torch.cuda._sleep(cycles)
        case.load()
    t0 = time.perf_counter()
    rc = case.call(S.cuda_stream)
    dt = (time.perf_counter() - t0) * 1e3
    if name not in HOST_RESULT:
        busy = not S.query()
        HOST_TIMES[name] = max(dt, HOST_TIMES.get(name, 0.0))
        assert busy, f"{name}: the caller's stream was idle when the call returned (it waited for the stream)"
        assert dt < ms / 2, f"{name}: the call took {dt:.1f} ms on the host behind a {ms:.0f} ms delay (it synchronised)"
    return rc


def _warm(case, S):
    torch = _torch()
    with torch.cuda.stream(S):
        case.load()
    _ok(case.call(S.cuda_stream))
    S.synchronize()


def _hooks(seams):
    L = _L()
    L.vga_testing_gc_encoder_segments_this_thread(12 if seams else 0)
    L.vga_testing_force_open_seams_this_thread(1 if seams else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROWS) + [n + "[seams]" for n in sorted(SEAM_ROWS)])
def test_device_entry_point_on_a_busy_stream(name, delay):
    torch = _torch()
    seams = name.endswith("[seams]")
    ep = name[:-len("[seams]")] if seams else name
    make = SEAM_ROWS[ep] if seams else ROWS[ep]
    shared = {}
    S = torch.cuda.Stream()
    _hooks(seams)
    try:
        _warm(make(0, shared), S)
        case = make(0, shared)
        rc = _run_on_busy_stream(ep, case, S, delay)
        S.synchronize()
        _ok(rc)
        case.check()
    finally:
        _hooks(False)
        torch.cuda.synchronize()
        if "ragged" in shared:
            shared["ragged"].close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CONCURRENT)
def test_two_calls_in_flight(name, delay):
    """call A waits on stream A behind the delay; call B, enqueued afterwards on stream B without one, runs first"""
    torch = _torch()
    shared = {}
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        _warm(ROWS[name](0, shared), A)
        _warm(ROWS[name](1, shared), B)
        a, b = ROWS[name](0, shared), ROWS[name](1, shared)
        rc_a = _run_on_busy_stream(name, a, A, delay)
        with torch.cuda.stream(B):
            b.poison()
            b.load()
        rc_b = b.call(B.cuda_stream)
        B.synchronize()
        assert not A.query(), f"{name}: stream A finished before call B had run (the delay is too short to overlap)"
        A.synchronize()
        _ok(rc_a)
        _ok(rc_b)
        a.check()
        b.check()
    finally:
        torch.cuda.synchronize()
        if "ragged" in shared:
            shared["ragged"].close()

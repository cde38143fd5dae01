"""The codec *_device entry points at the loosest buffer layout include/vgaudio_hip.h allows.

Every other GPU test hands the codecs rows on 256-byte boundaries with pitches rounded up to 16 bytes.  Here a batch's rows
lie inside a LARGER allocation -- 256 bytes of guard, three foreign rows, the rows, three foreign rows, 256 bytes of guard,
everything but the batch's own samples seeded junk -- at the minimum the header promises: the base at each residue the
contract allows, the smallest legal pitch that is no multiple of the kernels' vector width, and the view a caller gets from
rows [3, 3 + m) of a batch with that pitch.  One buffer leaves the aligned layout per case (a failure names its buffer), plus
`both` for all of them at once.  Every output is compared with the oracle byte for byte; an input allocation may not change
at all, an output allocation not outside [base, base + nrows * pitch) (and not in its padding columns where that is promised).
The guards keep a kernel's clamped over-read inside the allocation: the point is wrong bytes, not faults.

The ADX cases also assert WHICH kernel form ran (vga_testing_adx_last_path_this_thread); one layout just outside each
contract must be refused with VGA_ERR_ARGUMENT and leave the output alone.  vga_dsp_write_device and vga_genh_read_device,
two container calls that take the codec's rows, are placed the same way; the other container calls are placed by
test_gpu_container_layouts.py (ELSEWHERE below), and ALIGNED_ONLY, the list of calls no test moves, is empty.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from test_gpu_device_streams import header_device_entry_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256
ERR_ARGUMENT = -1

# ====================================================================== the CPU check: every device entry point has a home
# the calls this file places off alignment (or refuses just outside their contract)
HERE = {
    "vga_gcadpcm_coefs_device": "test_gc_coefs", "vga_gcadpcm_encode_device": "test_gc_encode",
    "vga_gcadpcm_decode_device": "test_gc_decode", "vga_gcadpcm_build_channels_device": "test_gc_build_channels",
    "vga_gcadpcm_coefs_device_v": "test_refuses_ragged_buffers_at_8_mod_16",
    "vga_gcadpcm_encode_device_v": "test_refuses_ragged_buffers_at_8_mod_16",
    "vga_gcadpcm_decode_device_v": "test_refuses_ragged_buffers_at_8_mod_16",   # the layout is the handle's, only the base the caller's
    "vga_dsp_write_device": "test_dsp_write", "vga_genh_read_device": "test_genh_read",
    "vga_adx_encode_device": "test_adx_encode", "vga_adx_decode_device": "test_adx_decode",
    "vga_hca_encode_device": "test_hca_encode", "vga_hca_decode_device": "test_hca_decode",
    "vga_adx_crypt_device": "test_adx_crypt", "vga_adx_find_key_device": "test_adx_find_key",
    "vga_hca_crypt_device": "test_hca_crypt", "vga_hca_find_key_device": "test_hca_find_key",
    "vga_hca_byte_position_counts_device": "test_hca_byte_position_counts",
}
# calls that another file's test already moves off alignment: (file, test, what it moves).  The call's name occurs in that file
ELSEWHERE = {
    "vga_dsp_read_device": ("test_gpu_container_readers.py", "test_dsp_device_read_equals_host_read",
                            "images at every offset mod 16, file pitches of the image size + offset + 3, row pitches off 16"),
    "vga_adx_read_device": ("test_gpu_container_readers.py", "test_adx_device_read_equals_host_read_every_residue",
                            "images at every offset mod 16, file and row pitches off 16, both kernels"),
    "vga_hca_read_device": ("test_gpu_container_readers.py", "test_hca_device_read_equals_host_read",
                            "images at every offset mod 16, file pitches of the image size + offset"),
    "vga_wave_deinterleave_pcm16_device": ("test_gpu_wave.py", "test_unaligned_data_chunk_on_device", "the data chunk 3 bytes in"),
    "vga_wave_write_pcm16_device": ("test_gpu_wave.py", "test_unaligned_data_chunk_on_device", "the image 1 byte in"),
    # test_gpu_container_layouts.py: the container calls, placed as this file places the codecs
    "vga_nwstm_write_device": ("test_gpu_container_layouts.py", "test_nwstm_write",
                               "ADPCM rows and images at bases 1, 2, 4, 8 and pitches off 16, the seek table and the small arrays a short in"),
    "vga_nwstm_read_device": ("test_gpu_container_layouts.py", "test_nwstm_read",
                              "images at bases 1, 2, 4, 8 on an odd pitch, rows at bases 1, 2, 4, 8 and pitches off 16"),
    "vga_hps_write_device": ("test_gpu_container_layouts.py", "test_hps_write",
                             "as the NW writer, and the PCM rows behind the block histories a sample in on an odd pitch"),
    "vga_hps_read_device": ("test_gpu_container_layouts.py", "test_hps_read", "as the NW reader"),
    "vga_idsp_write_device": ("test_gpu_container_layouts.py", "test_idsp_write", "as the NW writer, the small arrays a short in"),
    "vga_idsp_read_device": ("test_gpu_container_layouts.py", "test_idsp_read", "as the NW reader"),
    "vga_adx_write_device": ("test_gpu_container_layouts.py", "test_adx_write",
                             "audio at an odd base on an odd pitch, the histories a short in, the image at bases 1, 2, 4, 8"),
    "vga_hca_write_device": ("test_gpu_container_layouts.py", "test_hca_write", "frames and images at odd bases on odd pitches"),
    "vga_synth_pcm16_device": ("test_gpu_container_layouts.py", "test_synth_pcm16",
                               "rows a sample in on an odd pitch, the parameters a uint32 in"),
}
# NOT COVERED off alignment: calls whose buffers no test anywhere moves; (file, test) is the test that runs the call on
# torch allocations (256-byte bases) with rounded pitches.  Empty since test_gpu_container_layouts.py: a new device entry
# point belongs in HERE or ELSEWHERE, not here.
ALIGNED_ONLY = {}


def _function_body(text, test):
    """the source of top-level function `test` in `text`, decorators aside; None when there is none"""
    m = re.search(r"^def " + test + r"\(.*?(?=^\S|\Z)", text, flags=re.M | re.S)
    return m and m.group(0)


def test_every_device_entry_point_has_a_layout_test():
    declared = header_device_entry_points()
    assert len(declared) >= 32
    tables = (HERE, ELSEWHERE, ALIGNED_ONLY)
    listed = [name for t in tables for name in t]
    assert len(listed) == len(set(listed)), sorted(n for n in set(listed) if listed.count(n) > 1)
    assert set(listed) == declared, (sorted(declared - set(listed)), sorted(set(listed) - declared))
    own = open(os.path.abspath(__file__)).read()
    for name, test in HERE.items():                              # the named test itself makes the call
        body = _function_body(own, test)
        assert body, (name, test)
        assert re.search(r"\b" + name + r"\(", body), (name, test)
    for name, entry in {**ELSEWHERE, **ALIGNED_ONLY}.items():     # the named file has the test and makes the call
        text = open(os.path.join(ROOT, "tests", entry[0])).read()
        assert _function_body(text, entry[1]), (name, entry)
        assert re.search(r"\b" + name + r"\(", text), (name, entry)
    for name, (path, test, what) in ELSEWHERE.items():
        assert what


# ====================================================================== helpers (GPU only below this line)
def _torch():
    import torch
    return torch


def _L():
    from vgaudio_amd import _lib
    return _lib.lib()


def _po():
    from oracle import pyoracle as po
    return po


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _err():
    return _L().vga_last_error().decode(errors="replace")


def _ok(rc):
    assert rc == 0, f"rc {rc}: {_err()}"


def _up(a):
    return _torch().from_numpy(np.array(a, order="C")).cuda()           # a copy: the shared references are read-only


def _round_up(v, m):
    return (v + m - 1) // m * m


_SEED = [0]


class Placed:
    """a batch's rows inside a larger device allocation; see place()"""

    def __init__(self, rows, pitch, base_off, dtype, view=False, offsets=None, extent=None):
        torch = _torch()
        self.dtype = np.dtype(dtype)
        isz = self.dtype.itemsize
        if isinstance(rows, tuple):                              # an output: (nrows, width), junk where the samples go
            self.nrows, self.width = rows
            data = None
        else:
            data = [np.ascontiguousarray(r, dtype=self.dtype) for r in rows]
            self.nrows, self.width = len(data), len(data[0])
        pb = pitch * isz
        self.pitch = pitch
        self.offs = (np.arange(self.nrows, dtype=np.int64) * pb) if offsets is None else np.asarray(offsets, np.int64) * isz
        self.ext = int(self.nrows * pb if extent is None else extent * isz)
        assert offsets is not None or pitch >= self.width
        assert int(self.offs[-1]) + self.width * isz <= self.ext
        foreign = 3 * max(pb, 16)
        if view:                                                 # rows [3, 3 + m) of a batch that begins on a 256-byte boundary
            assert offsets is None and base_off is None
            self.base = GUARD + 3 * pb
        else:
            self.base = _round_up(GUARD + foreign, 256) + base_off
        total = self.base + self.ext + foreign + GUARD
        _SEED[0] += 1
        self.before = np.random.default_rng(0xA11C + _SEED[0]).integers(0, 256, total, dtype=np.uint8)
        self.own = np.zeros(total, bool)
        for r in range(self.nrows):
            at = self.base + int(self.offs[r])
            self.own[at:at + self.width * isz] = True
            if data is not None:
                self.before[at:at + self.width * isz] = data[r].view(np.uint8)
        self.t = torch.from_numpy(self.before.copy()).cuda()
        assert self.t.data_ptr() % 256 == 0
        self.ptr = self.t.data_ptr() + self.base
        self.got = None

    def fetch(self):
        self.got = self.t.cpu().numpy()
        return self

    def rows(self):
        """the batch's rows as the call left them"""
        if self.got is None:
            self.fetch()
        isz = self.dtype.itemsize
        return np.stack([self.got[self.base + int(o):self.base + int(o) + self.width * isz].copy().view(self.dtype) for o in self.offs])

    def _same(self, mask, what):
        if self.got is None:
            self.fetch()
        bad = np.flatnonzero((self.got != self.before) & mask)
        assert bad.size == 0, (f"{what}: {bad.size} bytes changed, first {int(bad[0]) - self.base} bytes from the base "
                               f"(rows span {self.ext} bytes, pitch {self.pitch * self.dtype.itemsize})")

    def unchanged(self, what):
        """an input: no byte of the allocation may change"""
        self._same(np.ones(self.before.size, bool), what + " (input)")

    def kept(self, what, padding=False):
        """an output: nothing outside [base, base + extent) changed; padding=True: nor any byte that is not a sample"""
        if padding:
            mask = ~self.own
        else:
            mask = np.ones(self.before.size, bool)
            mask[self.base:self.base + self.ext] = False
        self._same(mask, what + " (output)")


def place(rows, pitch, base_off, dtype, **kw):
    """rows (arrays, or (nrows, width) for an output) -> Placed: .ptr is what to pass, .unchanged() / .kept() the checker.
    Layout: GUARD bytes, three foreign rows, the rows base_off bytes past a 256-byte boundary with `pitch` elements between
    them, three foreign rows, GUARD bytes; base_off=None with view=True: the rows are rows 3.. of a batch on a boundary."""
    return Placed(rows, pitch, base_off, dtype, **kw)


def small(values, shift, dtype):
    """a per-channel array `shift` elements into a junk-filled allocation"""
    v = np.ascontiguousarray(values, dtype=dtype).reshape(-1)
    return place([v], len(v), shift * v.dtype.itemsize, dtype)


def _eq(got, want, what):
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} elements differ from the oracle, first at {bad[0].tolist()}")


def _pick(layouts, name):
    """layouts: {buffer: {layout name: (pitch, base_off) or 'view'}}; case `buf:layout` moves one buffer, `both` all"""
    out = {}
    for buf, table in layouts.items():
        if name == "both":
            out[buf] = table["both"]
        elif name.split(":")[0] == buf:
            out[buf] = table[name.split(":")[1]]
        else:
            out[buf] = table["aligned"]
    return out


def _put(rows, spec, dtype, **kw):
    pitch, off = spec
    return place(rows, pitch, None if off == "view" else off, dtype, view=off == "view", **kw)


def _case_names(layouts, extra=()):
    names = ["aligned"]
    for buf, table in layouts.items():
        names += [f"{buf}:{k}" for k in table if k not in ("aligned", "both")]
    return names + list(extra) + ["both"]


# ====================================================================== GC-ADPCM
GC_NCH = [1, 9, 70]


def _gc():
    import gc_packed_sum_cases as g
    return g


def _gc_n():
    return 14 * 600 + 5


def _gc_nb():
    n = _gc_n()
    return n // 14 * 8 + (1 + (n % 14 + 1) // 2 if n % 14 else 0)


def _not_multiple(p, step, m):
    """the smallest legal pitch >= p (legal: multiples of step) that is no multiple of m"""
    p = _round_up(p, step)
    return p + step if p % m == 0 else p


# PCM under GC: base 4-byte aligned, pitch even; vector width 16 bytes = 8 samples
GC_PCM = {"aligned": (_round_up(_gc_n(), 8), 0), "base4": (_round_up(_gc_n(), 8), 4), "base8": (_round_up(_gc_n(), 8), 8),
          "base12": (_round_up(_gc_n(), 8), 12), "min_pitch": (_not_multiple(_gc_n(), 2, 8), 0),
          "both": (_not_multiple(_gc_n(), 2, 8), "view")}
# GC ADPCM: base 8-byte aligned, pitch a multiple of 8; vector width 16 bytes
GC_ADPCM = {"aligned": (_round_up(_gc_nb(), 16), 0), "base8": (_round_up(_gc_nb(), 16), 8),
            "min_pitch": (_not_multiple(_gc_nb(), 8, 16), 0), "both": (_not_multiple(_gc_nb(), 8, 16), "view")}


def test_the_gc_layouts_are_the_contract_minimum():
    """(CPU) the tables above are what they claim: legal, and off the vector width"""
    assert _gc_nb() == _po().gc_sample_count_to_byte_count(_gc_n()) and _gc_n() == _gc().N
    p, _ = GC_PCM["min_pitch"]
    assert p % 2 == 0 and p % 8 != 0 and p >= _gc_n() and (3 * p * 2) % 4 == 0 and (3 * p * 2) % 16 != 0
    p, _ = GC_ADPCM["min_pitch"]
    assert p % 8 == 0 and p % 16 == 8 and p >= _gc_nb() and (3 * p) % 16 == 8


class _Hooks:
    """test hooks of the calling thread, restored on exit"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        L = _L()
        self.fns = {"segments": L.vga_testing_gc_encoder_segments_this_thread, "layout": L.vga_testing_gc_encoder_layout_this_thread,
                    "persistent": L.vga_testing_gc_encoder_persistent_this_thread, "coefs": L.vga_testing_gc_coefs_variant_this_thread}
        self.old = {k: self.fns[k](v) for k, v in self.kw.items()}

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.fns[k](v)


@functools.lru_cache(maxsize=None)
def _gc_own_coefs():
    po = _po()
    pcm = _gc().cases()[0]
    out = np.stack([po.gc_calculate_coefficients(pcm[c]) for c in range(pcm.shape[0])])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _gc_decoded():
    po = _po()
    pcm, coefs, h1, h2, want, end = _gc().cases()
    out = np.stack([po.gc_decode(want[c], coefs[c], _gc_n(), hist1=int(h1[c]), hist2=int(h2[c])) for c in range(pcm.shape[0])])
    out.setflags(write=False)
    return out


GC_COEFS_LAYOUTS = {"pcm": GC_PCM}


@pytest.mark.gpu
@pytest.mark.parametrize("layout", _case_names(GC_COEFS_LAYOUTS, extra=["small"]))
@pytest.mark.parametrize("nch", GC_NCH)
def test_gc_coefs(nch, layout):
    """vga_gcadpcm_coefs_device: every coefficient kernel at min_pitch and both, the launcher's choice elsewhere"""
    torch = _torch()
    L = _L()
    n = _gc_n()
    pcm = _gc().cases()[0][:nch]
    spec = _pick(GC_COEFS_LAYOUTS, layout)
    wsb = L.vga_gcadpcm_coefs_workspace_bytes(nch, n)
    for variant in ((0, 1, 2, 3) if layout in ("pcm:min_pitch", "both") else (0,)):
        d_pcm = _put(pcm, spec["pcm"], np.int16)
        d_coefs = place((1, nch * 16), nch * 16, 32 if layout in ("small", "both") else 0, np.int16)
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
        with _Hooks(coefs=variant):
            _ok(L.vga_gcadpcm_coefs_device(d_pcm.ptr, d_pcm.pitch, nch, n, d_coefs.ptr, ws.data_ptr(), ws.numel(), _stream()))
        torch.cuda.synchronize()
        _eq(d_coefs.rows().reshape(nch, 16), _gc_own_coefs()[:nch], f"coefs (variant {variant})")
        d_pcm.unchanged("pcm")
        d_coefs.kept("coefs", padding=True)


GC_ENCODE_LAYOUTS = {"pcm": GC_PCM, "adpcm": GC_ADPCM}


@pytest.mark.gpu
@pytest.mark.parametrize("layout", _case_names(GC_ENCODE_LAYOUTS, extra=["small"]))
@pytest.mark.parametrize("nch", GC_NCH)
def test_gc_encode(nch, layout):
    """vga_gcadpcm_encode_device on the packed-sum channels (cold block, 64-bit keys) with their coefficients and histories;
    `both` under every combination of pieces, lane layout and workgroup scheme, the rest with three pieces"""
    torch = _torch()
    L = _L()
    n, nb = _gc_n(), _gc_nb()
    pcm, coefs, h1, h2, want, _ = _gc().cases()
    spec = _pick(GC_ENCODE_LAYOUTS, layout)
    shifted = layout in ("small", "both")
    hooks = ([dict(segments=s, layout=w, persistent=p) for s in (1, 3) for w in (4, 8) for p in (1, 2)] if layout == "both"
             else [dict(segments=3)])
    for hook in hooks:
        d_pcm = _put(pcm[:nch], spec["pcm"], np.int16)
        d_out = _put((nch, nb), spec["adpcm"], np.uint8)
        d_coefs = small(coefs[:nch], 16 if shifted else 0, np.int16)          # 32 bytes in
        d_h1, d_h2 = small(h1[:nch], 1 if shifted else 0, np.int16), small(h2[:nch], 1 if shifted else 0, np.int16)
        with _Hooks(**hook):
            _ok(L.vga_gcadpcm_encode_device(d_pcm.ptr, d_pcm.pitch, nch, n, d_coefs.ptr, d_h1.ptr, d_h2.ptr, d_out.ptr, d_out.pitch,
                                            _stream()))
        torch.cuda.synchronize()
        _eq(d_out.rows(), want[:nch], f"adpcm {hook}")
        d_out.kept("adpcm")
        for p, what in ((d_pcm, "pcm"), (d_coefs, "coefs"), (d_h1, "hist1"), (d_h2, "hist2")):
            p.unchanged(what)


GC_DECODE_LAYOUTS = {"adpcm": GC_ADPCM, "pcm": GC_PCM}


@pytest.mark.gpu
@pytest.mark.parametrize("layout", _case_names(GC_DECODE_LAYOUTS, extra=["small"]))
@pytest.mark.parametrize("nch", GC_NCH)
def test_gc_decode(nch, layout):
    """vga_gcadpcm_decode_device: the input side (rows read as 16- and 8-byte vectors from rows that are only 8-byte aligned)
    and the output side at three pieces; the columns >= n of the PCM rows stay as they were.  The output side over several
    pieces of a long channel is test_gpu_gcadpcm.py::test_decode_into_rows_that_are_only_dword_aligned."""
    torch = _torch()
    L = _L()
    n = _gc_n()
    pcm, coefs, h1, h2, want, end = _gc().cases()
    spec = _pick(GC_DECODE_LAYOUTS, layout)
    shifted = layout in ("small", "both")
    d_in = _put(want[:nch], spec["adpcm"], np.uint8)
    d_out = _put((nch, n), spec["pcm"], np.int16)
    d_coefs = small(coefs[:nch], 16 if shifted else 0, np.int16)
    d_h1, d_h2 = small(h1[:nch], 1 if shifted else 0, np.int16), small(h2[:nch], 1 if shifted else 0, np.int16)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    with _Hooks(segments=3):
        _ok(L.vga_gcadpcm_decode_device(d_in.ptr, d_in.pitch, d_coefs.ptr, nch, n, d_h1.ptr, d_h2.ptr, d_out.ptr, d_out.pitch,
                                        status.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [0, 0, 0, 0]
    got = d_out.rows()
    _eq(got, _gc_decoded()[:nch], "pcm")
    _eq(got[:, -2:], end[:nch], "end histories")
    d_out.kept("pcm", padding=True)
    for p, what in ((d_in, "adpcm"), (d_coefs, "coefs"), (d_h1, "hist1"), (d_h2, "hist2")):
        p.unchanged(what)


@functools.lru_cache(maxsize=None)
def _build_channels_case():
    po = _po()
    n, loop, alignment, spe, nch = 3000, (100, 2900), 1000, 0x200, 5
    pcm = po.synth_generate(nch, n)
    coefs, adpcm = po.gc_encode_batch(pcm)
    op = po.gc_channel_params(n, True, loop[0], loop[1], alignment, spe)
    want = [po.gc_build_channel(adpcm[c], coefs[c], op) for c in range(nch)]
    return n, loop, alignment, spe, nch, np.asarray(coefs).reshape(nch, 16), np.asarray(adpcm), want


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["aligned", "min"])
def test_gc_build_channels(layout):
    """vga_gcadpcm_build_channels_device on the (3000, (100, 2900), 1000, 0x200) case of test_build_channels_matches_oracle:
    ADPCM in and out at base 8 / pitch 8 mod 16, PCM out at base 4 / an even pitch off 8, the seek table on an odd pitch at
    an odd element, loop contexts and coefficients shifted, the workspace at its 16 bytes"""
    from vgaudio_amd import _lib
    torch = _torch()
    L = _L()
    po = _po()
    n, loop, alignment, spe, nch, coefs, adpcm, want = _build_channels_case()
    lay = want[0][1]
    ns, ne = lay.sample_count_aligned, lay.seek_table_entries
    na = po.gc_sample_count_to_byte_count(ns)
    nb = adpcm.shape[1]
    low = layout == "min"
    p = _lib.GcChannelParamsC(n, 1, loop[0], loop[1], alignment, spe)
    d_in = place(adpcm, _not_multiple(nb, 8, 16) if low else _round_up(nb, 16), 8 if low else 0, np.uint8)
    a_out = place((nch, na), _not_multiple(na, 8, 16) if low else _round_up(na, 16), 8 if low else 0, np.uint8)
    p_out = place((nch, ns), _not_multiple(ns, 2, 8) if low else _round_up(ns, 8), 4 if low else 0, np.int16)
    s_out = place((nch, 2 * ne), (2 * ne) | 1 if low else _round_up(2 * ne, 8), 2 if low else 0, np.int16)
    c_out = place((1, nch * 3), nch * 3, 2 if low else 0, np.int16)
    d_coefs = small(coefs, 16 if low else 0, np.int16)
    wsb = L.vga_gcadpcm_build_channels_workspace_bytes(nch, C.byref(p))
    ws = torch.empty(wsb + 512, dtype=torch.uint8, device="cuda")
    ws_ptr = _round_up(ws.data_ptr(), 256) + (16 if low else 0)
    _ok(L.vga_gcadpcm_build_channels_device(d_in.ptr, d_in.pitch, d_coefs.ptr, nch, C.byref(p), a_out.ptr, a_out.pitch, p_out.ptr,
                                            p_out.pitch, s_out.ptr, s_out.pitch, c_out.ptr, ws_ptr, wsb, _stream()))
    torch.cuda.synchronize()
    ga, gp, gs, gc = a_out.rows(), p_out.rows(), s_out.rows(), c_out.rows().reshape(nch, 3)
    for c in range(nch):
        rc, _, wa, wp, wsk, wctx = want[c]
        assert rc == 0
        _eq(ga[c], wa, f"adpcm {c}")
        _eq(gp[c], wp, f"pcm {c}")
        _eq(gs[c], wsk, f"seek {c}")
        _eq(gc[c], wctx, f"loop context {c}")
    for q, what in ((a_out, "adpcm out"), (p_out, "pcm out"), (s_out, "seek out")):
        q.kept(what)
    c_out.kept("loop context", padding=True)
    d_in.unchanged("adpcm in")
    d_coefs.unchanged("coefs")


# ====================================================================== the two container calls nothing else moves
DSP_WRITE_CASES = ["aligned", "adpcm:base8", "adpcm:min_pitch", "file:base8", "small", "both"]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", DSP_WRITE_CASES)
@pytest.mark.parametrize("nch", [1, 2, 5])
def test_dsp_write(nch, layout):
    """vga_dsp_write_device, a looping file with gains and both contexts: ADPCM rows at base 8 / pitch 8 mod 16 as the
    codec's contract allows, the image at its 8-byte minimum (with five channels the audio then starts 8 mod 16 once more)"""
    from vgaudio_amd import _lib
    torch = _torch()
    L = _L()
    po = _po()
    n, nb = _gc_n(), _gc_nb()
    _, coefs, _, _, adpcm, _ = _gc().cases()
    rng = np.random.default_rng(40 + nch)
    gain = rng.integers(-32768, 32768, nch).astype(np.int16)
    sc, lc = rng.integers(-32768, 32768, (nch, 3)).astype(np.int16), rng.integers(-32768, 32768, (nch, 3)).astype(np.int16)
    args = (48000, n, 1, 140, 8000, 14 * 64, 1, 0)
    rc, want = po.dsp_write(list(adpcm[:nch]), coefs[:nch], po.dsp_params(*args), gain=gain, start_context=sc, loop_context=lc)
    assert rc == 0
    p = _lib.DspParamsC(*args)
    lay = _lib.DspLayoutC()
    _ok(L.vga_dsp_layout_for(C.byref(p), nch, C.byref(lay)))
    assert lay.file_size == len(want)
    spec = _pick({"adpcm": GC_ADPCM}, layout)["adpcm"]
    shifted = layout in ("small", "both")
    d_in = _put(adpcm[:nch], spec, np.uint8)
    d_file = place((1, lay.file_size), lay.file_size, 8 if layout in ("file:base8", "both") else 0, np.uint8)
    d_coefs = small(coefs[:nch], 16 if shifted else 0, np.int16)
    d_gain, d_sc, d_lc = (small(v, 1 if shifted else 0, np.int16) for v in (gain, sc, lc))
    _ok(L.vga_dsp_write_device(d_in.ptr, d_in.pitch, nb, d_coefs.ptr, d_gain.ptr, d_sc.ptr, d_lc.ptr, nch, C.byref(p), d_file.ptr,
                               _stream()))
    torch.cuda.synchronize()
    _eq(d_file.rows()[0], np.asarray(want, dtype=np.uint8), "image")
    d_file.kept("image", padding=True)
    for q, what in ((d_in, "adpcm"), (d_coefs, "coefs"), (d_gain, "gain"), (d_sc, "start context"), (d_lc, "loop context")):
        q.unchanged(what)


GENH_READ_CASES = ["aligned", "files:base1", "files:odd_pitch", "rows:base1", "rows:odd_pitch", "both"]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", GENH_READ_CASES)
@pytest.mark.parametrize("interleave", [0x40, 6])
@pytest.mark.parametrize("nch", [1, 2])
def test_genh_read(nch, interleave, layout):
    """vga_genh_read_device, three images per call: the header states no alignment, so images and rows lie at any byte
    on any pitch; the read picks its granule from what it finds.  Rows equal Interleave.cs's DeInterleave restated in
    gc_containers_ref, as test_gpu_gc_containers.py holds the host read to it."""
    import gc_containers_ref as ref
    from vgaudio_amd.genh import parse
    torch = _torch()
    nf, n = 3, 14 * 300 + 5
    ab = ref.bytes_of(n)
    rng = np.random.default_rng(50 + nch)
    audio = rng.integers(0, 256, (nf, nch, ab)).astype(np.uint8)
    coefs = rng.integers(-32768, 32768, (nch, 16)).tolist()
    images = [np.frombuffer(ref.genh_image(48000, [audio[f, c].tobytes() for c in range(nch)], coefs, interleave, -1, n, 0), np.uint8)
              for f in range(nf)]
    info = parse(images[0].tobytes())
    assert info.adpcm_bytes == ab and info.channel_count == nch
    want = np.stack([np.frombuffer(r, np.uint8) for f in range(nf)
                     for r in ref.deinterleave(images[f][info.audio_data_offset:].tobytes(), ab * nch, interleave, nch)])
    size = len(images[0])
    fp, foff = _round_up(size, 16), 0
    if layout in ("files:odd_pitch", "both"):
        fp = size | 1
    if layout in ("files:base1", "both"):
        foff = 1
    rows = {"rows:base1": (_round_up(ab, 16), 1), "rows:odd_pitch": (ab | 1, 0), "both": (ab | 1, "view")}.get(layout, (_round_up(ab, 16), 0))
    d_files = place(images, fp, foff, np.uint8)
    d_rows = _put((nf * nch, ab), rows, np.uint8)
    _ok(_L().vga_genh_read_device(C.byref(info), d_files.ptr, fp, nf, d_rows.ptr, d_rows.pitch, _stream()))
    torch.cuda.synchronize()
    _eq(d_rows.rows(), want, "rows")
    d_rows.kept("rows")
    d_files.unchanged("files")


# ====================================================================== ADX
ADX_NCH = [1, 70]
ADX_N = 32 * 300 + 13
ADX_SETS = [dict(type=3), dict(type=4, version=3), dict(type=2, filter=2), dict(type=3, padding=24), dict(type=3, frame_size=34)]
PATH_PIECES, PATH_GENERAL = 1, 2


def _adx_params(**kw):
    from vgaudio_amd import _lib
    p = _lib.AdxParams()
    _L().vga_adx_default_params(C.byref(p))
    for key, v in kw.items():
        setattr(p, key, v)
    return p, _po().adx_params(**kw)


@functools.lru_cache(maxsize=None)
def _adx_case(k):
    """set k: (pcm [70, n], the oracle's bytes, its histories, its decode of those bytes)"""
    po = _po()
    pcm = po.synth_generate(ADX_NCH[-1], ADX_N, first_channel=300)
    _, op = _adx_params(**ADX_SETS[k])
    adx, hist = po.adx_encode_batch(pcm, op)
    dec = po.adx_decode_batch(adx, ADX_N, op)
    out = (pcm, np.asarray(adx), np.asarray(hist), np.asarray(dec))
    for a in out:
        a.setflags(write=False)
    return out


def _adx_path():
    e, d = C.c_int(-1), C.c_int(-1)
    assert _L().vga_testing_adx_last_path_this_thread(C.byref(e), C.byref(d)) == 0
    return e.value, d.value


def _takes_pieces(kw):
    return kw.get("frame_size", 18) == 18 and 0 <= kw.get("padding", 0) <= 64


# ADX PCM: any sample boundary, any pitch >= n; the time-piece kernels want base % 16 == 0 and pitch % 8 == 0
ADX_PCM = {"aligned": (_round_up(ADX_N, 8), 0), "base2": (_round_up(ADX_N, 8), 2), "base4": (_round_up(ADX_N, 8), 4),
           "base8": (_round_up(ADX_N, 8), 8), "min_pitch": (ADX_N, 0), "even_pitch": (_round_up(ADX_N, 8) + 2, 0),
           "odd_pitch_base2": (ADX_N, 2), "both": (ADX_N, "view")}
assert ADX_N % 2 == 1


def _adx_data_layouts(nb, decode):
    """ADX data: encode -- base and pitch even; decode -- any byte.  The time-piece kernels want both multiples of 4"""
    t = {"aligned": (_round_up(nb, 16), 0), "base2": (_round_up(nb, 16), 2), "min_pitch": (_not_multiple(nb, 2, 4), 0),
         "both": (_not_multiple(nb, 2, 4), "view")}
    if decode:
        t.update({"base1": (_round_up(nb, 16), 1), "odd_pitch": (nb | 1, 0), "both": (nb | 1, "view")})
    return t


ADX_CASES = _case_names({"pcm": ADX_PCM, "data": _adx_data_layouts(18, True)}, extra=["small"])
ADX_ENCODE_CASES = [c for c in ADX_CASES if c not in ("data:base1", "data:odd_pitch")]
ADX_DECODE_CASES = [c for c in ADX_CASES if c != "small"]          # decode has no small per-channel array to shift


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ADX_ENCODE_CASES)
@pytest.mark.parametrize("nch", ADX_NCH)
def test_adx_encode(nch, layout):
    """vga_adx_encode_device, five parameter sets: each of launch_encode's four layout conditions violated alone sends the
    call to the general kernel (path 2), the aligned layout of an 18-byte-frame set takes the time pieces (path 1)"""
    torch = _torch()
    L = _L()
    for k, kw in enumerate(ADX_SETS):
        pcm, want, whist, _ = _adx_case(k)
        p, _ = _adx_params(**kw)
        nb = want.shape[1]
        spec = _pick({"pcm": ADX_PCM, "data": _adx_data_layouts(nb, False)}, layout)
        d_pcm = _put(pcm[:nch], spec["pcm"], np.int16)
        d_out = _put((nch, nb), spec["data"], np.uint8)
        d_hist = place((1, nch), nch, 2 if layout in ("small", "both") else 0, np.int16)
        with _Hooks(segments=3):
            _ok(L.vga_adx_encode_device(d_pcm.ptr, d_pcm.pitch, nch, ADX_N, C.byref(p), d_out.ptr, d_out.pitch, d_hist.ptr, _stream()))
        path = _adx_path()[0]
        torch.cuda.synchronize()
        _eq(d_out.rows(), want[:nch], f"adx {kw}")
        _eq(d_hist.rows().reshape(-1), whist[:nch], f"history_out {kw}")
        d_out.kept(f"adx {kw}")
        d_hist.kept(f"history_out {kw}", padding=True)
        d_pcm.unchanged(f"pcm {kw}")
        fast = _takes_pieces(kw) and layout in ("aligned", "small")
        assert path == (PATH_PIECES if fast else PATH_GENERAL), (kw, layout, path)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ADX_DECODE_CASES)
@pytest.mark.parametrize("nch", ADX_NCH)
def test_adx_decode(nch, layout):
    """vga_adx_decode_device on the oracle's bytes: ADX data at any byte (the general kernel reads bytes), PCM rows at any
    sample; the mirror conditions of launch_decode violated one at a time"""
    torch = _torch()
    L = _L()
    for k, kw in enumerate(ADX_SETS):
        _, adx, _, want = _adx_case(k)
        p, _ = _adx_params(**kw)
        nb = adx.shape[1]
        spec = _pick({"pcm": ADX_PCM, "data": _adx_data_layouts(nb, True)}, layout)
        d_in = _put(adx[:nch], spec["data"], np.uint8)
        d_out = _put((nch, ADX_N), spec["pcm"], np.int16)
        status = torch.zeros(4, dtype=torch.int32, device="cuda")
        with _Hooks(segments=3):
            _ok(L.vga_adx_decode_device(d_in.ptr, d_in.pitch, nb, nch, ADX_N, C.byref(p), d_out.ptr, d_out.pitch, status.data_ptr(),
                                        _stream()))
        path = _adx_path()[1]
        torch.cuda.synchronize()
        assert status.cpu().numpy().tolist() == [0, 0, 0, 0], kw
        _eq(d_out.rows(), want[:nch], f"pcm {kw}")
        d_out.kept(f"pcm {kw}")
        d_in.unchanged(f"adx {kw}")
        fast = _takes_pieces(kw) and layout == "aligned"
        assert path == (PATH_PIECES if fast else PATH_GENERAL), (kw, layout, path)


# ====================================================================== HCA
HCA_NCH = [1, 2, 6]
HCA_NS, HCA_N = 3, 1024 * 6 + 100


@functools.lru_cache(maxsize=None)
def _hca_case(nch):
    from vgaudio_amd import _lib
    po = _po()
    pcm = po.synth_generate(HCA_NS * nch, HCA_N, first_channel=1200).reshape(HCA_NS, nch, HCA_N)
    cfg = _lib.HcaParamsC(po.HCA_QUALITY["High"], 0, 0, nch, 48000, HCA_N, 0, 0, 0)
    info = _lib.HcaInfoC()
    _ok(_L().vga_hca_encoder_initialize(C.byref(cfg), C.byref(info)))
    rc, oinfo, frames = po.hca_encode_batch(pcm, po.hca_params(nch, HCA_N, quality="High"))
    assert rc == 0
    rc, dec = po.hca_decode_batch(oinfo, frames)
    assert rc == 0
    frames, dec = np.asarray(frames), np.asarray(dec)
    for a in (pcm, frames, dec):
        a.setflags(write=False)
    return pcm, info, frames, dec


def _hca_pcm(nch, layout, out, n):
    """(Placed, stream_pitch, ch_pitch) for the PCM of HCA_NS streams of nch channels"""
    cp = _round_up(n, 8)
    sp, off = nch * cp, 0
    if layout in ("pcm:odd_ch_pitch", "both"):
        cp = n | 1
        sp = nch * cp
    if layout in ("pcm:stream_pitch", "both"):
        sp = nch * cp + 3                                        # not a multiple of ch_pitch (nor of anything else)
    if layout in ("pcm:base2", "both"):
        off = 2                                                  # one sample in
    offsets = [s * sp + c * cp for s in range(HCA_NS) for c in range(nch)]
    rows = (HCA_NS * nch, n) if out else None
    return rows, dict(pitch=cp, base_off=off, offsets=offsets, extent=HCA_NS * sp), sp, cp


HCA_ENCODE_CASES = ["aligned", "pcm:odd_ch_pitch", "pcm:stream_pitch", "pcm:base2", "frames:pitch2", "frames:base1", "frames:base2",
                    "frames:base3", "both"]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", HCA_ENCODE_CASES)
@pytest.mark.parametrize("nch", HCA_NCH)
def test_hca_encode(nch, layout):
    """vga_hca_encode_device, one and two channels (the wave encoder) and six (the workgroup encoder): PCM at any sample,
    frames at any byte with an even pitch -- the lead-byte stores of both encoders"""
    torch = _torch()
    L = _L()
    pcm, info, want, _ = _hca_case(nch)
    fb = want.shape[1]
    _, kw, sp, cp = _hca_pcm(nch, layout, False, HCA_N)
    d_pcm = place(pcm.reshape(HCA_NS * nch, HCA_N), kw["pitch"], kw["base_off"], np.int16, offsets=kw["offsets"], extent=kw["extent"])
    fp = _round_up(fb, 16)
    if layout in ("frames:pitch2", "both"):
        fp = _not_multiple(fb, 2, 4)
    off = {"frames:base1": 1, "frames:base2": 2, "frames:base3": 3, "both": 3}.get(layout, 0)
    d_out = place((HCA_NS, fb), fp, off, np.uint8)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    _ok(L.vga_hca_encode_device(d_pcm.ptr, sp, cp, HCA_NS, HCA_N, C.byref(info), d_out.ptr, fp, status.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [0, 0, 0, 0]
    _eq(d_out.rows(), want, "frames")
    d_out.kept("frames")
    d_pcm.unchanged("pcm")


HCA_DECODE_CASES = ["aligned", "frames:min", "pcm:odd_ch_pitch", "pcm:stream_pitch", "pcm:base2", "both"]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", HCA_DECODE_CASES)
@pytest.mark.parametrize("nch", HCA_NCH)
def test_hca_decode(nch, layout):
    """vga_hca_decode_device: frames 4 bytes in on the smallest pitch the header allows, junk in the slack -- exactly the 8
    bytes it asks for with six channels (14336 bytes of frames), 9 and 10 with one and two (2387 and 4774 bytes, and the
    pitch a multiple of 4); PCM out on odd pitches at an odd sample"""
    torch = _torch()
    L = _L()
    _, info, frames, want = _hca_case(nch)
    fb = frames.shape[1]
    n = want.shape[2]
    low = layout in ("frames:min", "both")
    fp = _round_up(fb + 8, 4) if low else _round_up(fb + 8, 16)   # low: the smallest pitch the call accepts
    assert nch != 6 or fp == fb + 8 or not low                   # six channels: whole dwords of frames, so exactly 8 bytes
    d_in = place(frames, fp, 4 if low else 0, np.uint8)
    rows, kw, sp, cp = _hca_pcm(nch, layout, True, n)
    d_out = place(rows, kw["pitch"], kw["base_off"], np.int16, offsets=kw["offsets"], extent=kw["extent"])
    wsb = L.vga_hca_decode_workspace_bytes(C.byref(info), HCA_NS)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    _ok(L.vga_hca_decode_device(C.byref(info), d_in.ptr, fp, HCA_NS, d_out.ptr, sp, cp, ws.data_ptr(), wsb, status.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [0, 0, 0, 0]
    _eq(d_out.rows().reshape(HCA_NS, nch, n), want, "pcm")
    d_out.kept("pcm")
    d_in.unchanged("frames")


# ====================================================================== encryption
def _adx_keys():
    from vgaudio_amd import _lib
    keys = (_lib.AdxKeyC * 6)()
    for i, name in enumerate((b"GHM", b"GHMSC", b"karaage", b"mituba", b"morio", b"ranatus")):
        _ok(_L().vga_adx_key_from_string(name, C.byref(keys[i])))
    return keys


def _okey(key):
    return _po().AdxKey(key.seed, key.mult, key.inc)


CRYPT_CASES = ["aligned", "odd"]


def _odd(nbytes, layout):
    """(pitch, base offset) of a byte buffer: the control, or an odd pitch at an odd base"""
    return ((nbytes | 1) + 2, 1) if layout == "odd" else (_round_up(nbytes, 16), 0)


@pytest.mark.gpu
@pytest.mark.parametrize("etype", [8, 9])
@pytest.mark.parametrize("layout", CRYPT_CASES)
@pytest.mark.parametrize("nch", [1, 67])
def test_adx_crypt(nch, etype, layout):
    torch = _torch()
    po = _po()
    frames = 301
    audio = np.random.default_rng(70 + nch).integers(0, 256, (nch, 18 * frames)).astype(np.uint8)
    audio[:, 18 * 7:18 * 8] = 0                                  # an empty frame
    key = _adx_keys()[3]
    want = np.stack(po.adx_crypt(list(audio), _okey(key), etype))
    pitch, off = _odd(18 * frames, layout)
    d = place(audio, pitch, off, np.uint8)
    _ok(_L().vga_adx_crypt_device(d.ptr, pitch, 18 * frames, nch, C.byref(key), etype, 18, _stream()))
    torch.cuda.synchronize()
    _eq(d.rows(), want, "audio")
    d.kept("audio", padding=True)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", CRYPT_CASES)
def test_adx_find_key(layout):
    po = _po()
    nch, n = 3, 32 * 800
    pcm = po.synth_generate(nch, n, first_channel=77)
    audio, _ = po.adx_encode_batch(pcm, po.adx_params())
    keys = _adx_keys()
    target = 4
    enc = np.stack(po.adx_crypt(list(audio), _okey(keys[target]), 8))
    want = next(i for i in range(len(keys)) if po.adx_test_key(list(enc), _okey(keys[i]), 8))
    assert want == target
    nb = enc.shape[1]
    pitch, off = _odd(nb, layout)
    d = place(enc, pitch, off, np.uint8)
    idx = C.c_int(-7)
    _ok(_L().vga_adx_find_key_device(d.ptr, pitch, nb, nch, 8, 18, keys, len(keys), C.byref(idx), _stream()))
    assert idx.value == want
    d.unchanged("audio")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", CRYPT_CASES)
def test_hca_crypt(layout):
    from vgaudio_amd import _lib
    torch = _torch()
    po = _po()
    ns, fc, fs = 3, 37, 682
    frames = np.random.default_rng(80).integers(0, 256, (ns, fc * fs)).astype(np.uint8)
    rc, dec, enc = po.hca_key_tables(56, 123456789)
    want = np.stack([po.hca_crypt(frames[s], fs, enc) for s in range(ns)])
    pitch, off = _odd(fc * fs, layout)
    d = place(frames, pitch, off, np.uint8)
    _ok(_L().vga_hca_crypt_device(d.ptr, pitch, ns, fc, fs, enc.ctypes.data_as(_lib.u8p), _stream()))
    torch.cuda.synchronize()
    _eq(d.rows(), want, "frames")
    d.kept("frames", padding=True)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", CRYPT_CASES)
def test_hca_find_key(layout):
    from vgaudio_amd import _lib
    po = _po()
    nch, n = 2, 1024 * 14
    pcm = po.synth_generate(nch, n, first_channel=1200).reshape(1, nch, n)
    cfg = _lib.HcaParamsC(po.HCA_QUALITY["High"], 0, 0, nch, 48000, n, 0, 0, 0)
    info = _lib.HcaInfoC()
    _ok(_L().vga_hca_encoder_initialize(C.byref(cfg), C.byref(info)))
    rc, oinfo, frames = po.hca_encode_batch(pcm, po.hca_params(nch, n, quality="High"))
    assert rc == 0
    codes = [int(c) for c in np.random.default_rng(90).integers(1, 2 ** 56, 9)]
    tables = [po.hca_key_tables(56, c) for c in codes]
    true = 6
    enc = po.hca_crypt(frames[0], info.frame_size, tables[true][2]).reshape(-1, info.frame_size)
    dtabs = np.ascontiguousarray(np.stack([t[1] for t in tables]))
    want = po.hca_find_key(oinfo, enc, dtabs)
    assert want == true
    flat = enc.reshape(1, -1)
    d = place(flat, flat.shape[1], 1 if layout == "odd" else 0, np.uint8)
    idx = C.c_int(-7)
    _ok(_L().vga_hca_find_key_device(C.byref(info), d.ptr, info.frame_count, dtabs.ctypes.data_as(_lib.u8p), len(codes), C.byref(idx),
                                     _stream()))
    assert idx.value == want
    d.unchanged("frames")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", CRYPT_CASES)
def test_hca_byte_position_counts(layout):
    po = _po()
    ns, fc, fs = 5, 37, 100
    frames = np.random.default_rng(100).integers(0, 256, (ns, fc * fs)).astype(np.uint8)
    want = po.hca_byte_position_counts(frames, fs, 30)
    pitch, off = _odd(fc * fs, layout)
    d = place(frames, pitch, off, np.uint8)
    counts = np.zeros((30, 256), dtype=np.uint32)
    _ok(_L().vga_hca_byte_position_counts_device(d.ptr, pitch, ns, fc, fs, 30, counts.ctypes.data, _stream()))
    assert np.array_equal(counts, want)
    d.unchanged("frames")


# ====================================================================== refusals: one layout just outside each contract
def _refused(rcs, errs, word, outs):
    """VGA_ERR_ARGUMENT from every call, vga_last_error() names the problem, and no byte of any buffer changed"""
    _torch().cuda.synchronize()
    assert rcs and all(rc == ERR_ARGUMENT for rc in rcs), (rcs, errs)
    assert all(word in e for e in errs), (word, errs)
    for o in outs:
        o.unchanged(word)


def _gc_refused(pp, po_, ap, ao, word, pcm_calls):
    """encode and decode on PCM rows (pitch pp, base offset po_) and ADPCM rows (ap, ao), one of them illegal; the
    coefficient call too where the PCM is what is wrong"""
    torch = _torch()
    L = _L()
    n, nb, nch = _gc_n(), _gc_nb(), 9
    pcm, coefs, _, _, want, _ = _gc().cases()
    d_coefs = _up(coefs[:nch])
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    d_pcm, d_out = place(pcm[:nch], pp, po_, np.int16), place((nch, nb), ap, ao, np.uint8)
    rcs = [L.vga_gcadpcm_encode_device(d_pcm.ptr, pp, nch, n, d_coefs.data_ptr(), None, None, d_out.ptr, ap, _stream())]
    errs = [_err()]
    d_in, d_dec = place(want[:nch], ap, ao, np.uint8), place((nch, n), pp, po_, np.int16)
    rcs.append(L.vga_gcadpcm_decode_device(d_in.ptr, ap, d_coefs.data_ptr(), nch, n, None, None, d_dec.ptr, pp, status.data_ptr(), _stream()))
    errs.append(_err())
    outs = [d_out, d_dec]
    if pcm_calls:
        ws = torch.empty(max(L.vga_gcadpcm_coefs_workspace_bytes(nch, n), 16), dtype=torch.uint8, device="cuda")
        d_c = place((1, nch * 16), nch * 16, 0, np.int16)
        rcs.append(L.vga_gcadpcm_coefs_device(d_pcm.ptr, pp, nch, n, d_c.ptr, ws.data_ptr(), ws.numel(), _stream()))
        errs.append(_err())
        outs.append(d_c)
    _refused(rcs, errs, word, outs)


@pytest.mark.gpu
def test_refuses_gc_pcm_base_at_2_mod_4():
    _gc_refused(GC_PCM["aligned"][0], 2, *GC_ADPCM["aligned"], "4-byte aligned", True)


@pytest.mark.gpu
def test_refuses_odd_gc_pcm_pitch():
    _gc_refused(_gc_n() | 1, 0, *GC_ADPCM["aligned"], "pitch even", True)


@pytest.mark.gpu
def test_refuses_gc_adpcm_pitch_at_4_mod_8():
    ap = _round_up(_gc_nb(), 8) + 4
    _gc_refused(*GC_PCM["aligned"], ap, 0, "multiple of 8", False)


@pytest.mark.gpu
def test_refuses_container_adpcm_pitch_at_4_mod_8():
    """the two container calls that take the codec's ADPCM rows: channel metadata and the DSP writer"""
    from vgaudio_amd import _lib
    torch = _torch()
    L = _L()
    n, loop, alignment, spe, nch, coefs, adpcm, want = _build_channels_case()
    na = _po().gc_sample_count_to_byte_count(want[0][1].sample_count_aligned)
    bp = _lib.GcChannelParamsC(n, 1, loop[0], loop[1], alignment, spe)
    pitch_in = _round_up(adpcm.shape[1], 8) + 4
    d_in, b_out = place(adpcm, pitch_in, 0, np.uint8), place((nch, na), _round_up(na, 16), 0, np.uint8)
    d_coefs = _up(coefs)
    wsb = L.vga_gcadpcm_build_channels_workspace_bytes(nch, C.byref(bp))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    rcs = [L.vga_gcadpcm_build_channels_device(d_in.ptr, pitch_in, d_coefs.data_ptr(), nch, C.byref(bp), b_out.ptr, _round_up(na, 16),
                                               None, 0, None, 0, None, ws.data_ptr(), wsb, _stream())]
    errs = [_err()]
    dp = _lib.DspParamsC(48000, n, 0, 0, 0, 14 * 64, 1, 1)
    lay = _lib.DspLayoutC()
    _ok(L.vga_dsp_layout_for(C.byref(dp), nch, C.byref(lay)))
    d_file = place((1, lay.file_size), lay.file_size, 0, np.uint8)
    rcs.append(L.vga_dsp_write_device(d_in.ptr, pitch_in, adpcm.shape[1], d_coefs.data_ptr(), None, None, None, nch, C.byref(dp),
                                      d_file.ptr, _stream()))
    errs.append(_err())
    _refused(rcs, errs, "multiple of 8", [d_in, b_out, d_file])


@pytest.mark.gpu
def test_refuses_odd_adx_out_pitch():
    L = _L()
    nch = 9
    pcm, want, _, _ = _adx_case(0)
    p, _ = _adx_params(**ADX_SETS[0])
    nb = want.shape[1]
    pp = _round_up(ADX_N, 8)
    d_pcm, d_out, d_hist = place(pcm[:nch], pp, 0, np.int16), place((nch, nb), nb | 1, 0, np.uint8), place((1, nch), nch, 0, np.int16)
    rc = L.vga_adx_encode_device(d_pcm.ptr, pp, nch, ADX_N, C.byref(p), d_out.ptr, nb | 1, d_hist.ptr, _stream())
    _refused([rc], [_err()], "even", [d_out, d_hist, d_pcm])


@pytest.mark.gpu
def test_refuses_hca_decode_frames_at_2_mod_4():
    torch = _torch()
    L = _L()
    _, info, frames, dec = _hca_case(2)
    fb, n = frames.shape[1], dec.shape[2]
    fp, cp = _round_up(fb + 8, 16), _round_up(n, 8)
    d_in, d_out = place(frames, fp, 2, np.uint8), place((HCA_NS * 2, n), cp, 0, np.int16)
    wsb = L.vga_hca_decode_workspace_bytes(C.byref(info), HCA_NS)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    rc = L.vga_hca_decode_device(C.byref(info), d_in.ptr, fp, HCA_NS, d_out.ptr, 2 * cp, cp, ws.data_ptr(), wsb, status.data_ptr(), _stream())
    _refused([rc], [_err()], "4-byte alignment", [d_out, d_in])


@pytest.mark.gpu
def test_refuses_ragged_buffers_at_8_mod_16():
    """the _device_v calls take their layout from the handle; the caller's part is the 16-byte base of each packed buffer"""
    from vgaudio_amd.device import GcRaggedBatch
    torch = _torch()
    L = _L()
    r = GcRaggedBatch([1000, 14 * 30 + 3, 37], "cuda")
    try:
        ns, nb = int(r.pcm_samples), int(r.adpcm_bytes)
        d_pcm, d_ok_pcm = place((1, ns), ns, 8, np.int16), place((1, ns), ns, 0, np.int16)
        d_ad, d_ok_ad = place((1, nb), nb, 8, np.uint8), place((1, nb), nb, 0, np.uint8)
        d_c, d_c8 = place((1, r.nch * 16), r.nch * 16, 0, np.int16), place((1, r.nch * 16), r.nch * 16, 8, np.int16)
        ws = torch.empty(max(r.workspace_bytes, 16), dtype=torch.uint8, device="cuda")
        status = torch.zeros(4, dtype=torch.int32, device="cuda")
        rcs, errs = [], []
        for a, b in ((d_pcm, d_c), (d_ok_pcm, d_c8)):
            rcs.append(L.vga_gcadpcm_coefs_device_v(r.handle, a.ptr, b.ptr, ws.data_ptr(), ws.numel(), _stream()))
            errs.append(_err())
        for a, b in ((d_pcm, d_ok_ad), (d_ok_pcm, d_ad)):
            rcs.append(L.vga_gcadpcm_encode_device_v(r.handle, a.ptr, d_c.ptr, None, None, b.ptr, _stream()))
            errs.append(_err())
        for a, b in ((d_ad, d_ok_pcm), (d_ok_ad, d_pcm)):
            rcs.append(L.vga_gcadpcm_decode_device_v(r.handle, a.ptr, d_c.ptr, None, None, b.ptr, status.data_ptr(), _stream()))
            errs.append(_err())
        torch.cuda.synchronize()
    finally:
        r.close()
    _refused(rcs, errs, "16-byte aligned", [d_pcm, d_ad, d_ok_pcm, d_ok_ad, d_c, d_c8])

"""The container *_device entry points at the loosest buffer layout their headers allow.

test_gpu_device_layouts.py places the codecs' rows at the minimum include/vgaudio_hip.h promises; this file does the same
for the container writers and readers, the calls whose host side PICKS a kernel form from what it is handed:
interleave_images, deinterleave_images, launch_interleave, the HPS body and gather launches and the PCM (de)interleaves OR
every address, pitch, interleave and last-block size into one word and instantiate a 16-, 8-, 4-, 2- or 1-byte granule from
it (container::pick_granule).  The kernels then take it that the granule divides the interleave and the last block, move
ragged ends byte by byte and zero-fill what no block supplies.  gfx950 serves misaligned accesses, so a granule that is
merely too wide for its address returns the right bytes; what these cases can catch is arithmetic that assumes
divisibility (a granule across two channels or two blocks, a ragged end from the wrong place), a store outside the call's
own bytes (between two images, behind a row) and junk from behind a row where the reference has zeros.

Every case: inputs are Placed objects in seeded junk and may not change; outputs are junk-filled Placed objects, compared
with the restatement the suite already trusts (nwstm_ref, gc_containers_ref, nwstm_pcm_ref, nwwav_ref, oracle/pyref,
numpy) and then kept(padding=True): no byte that is not an image or row byte may differ, the bytes between two images and
behind a row included.  `aligned` is the control (256-byte base, rounded pitches), then one buffer at a time, then `both`:
everything at once, the rows a view of rows [3, 3 + m) of a larger batch.  Container writers only move bytes, so ADPCM
rows, coefficients, gains, contexts and seek tables are seeded random values; loops start at 0 (alignment_needed == 0).

Two CPU checks: every device call of vgaudio_hip_pcm.h and vgaudio_hip_nwwav.h has a test here, and for every call that
goes through pick_granule the cases reach every granule its geometry allows (GRANULE_CALLS states each cap).
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from test_gpu_device_layouts import (GUARD, ROOT, _eq, _err, _function_body, _L, _not_multiple, _ok, _pick, _put, _refused, _round_up,
                                     _stream, _torch, place, small)

S16, BYTES = 0, 1                                    # VGA_SAMPLES_S16, VGA_SAMPLES_8BIT
PCM8, PCM16 = 0, 1                                   # VGA_NW_CODEC_*

# ====================================================================== the CPU checks
# every vga_*_device call this file places off alignment -> the test that makes the call
HERE = {
    "vga_nwstm_write_device": "test_nwstm_write", "vga_nwstm_read_device": "test_nwstm_read",
    "vga_hps_write_device": "test_hps_write", "vga_hps_read_device": "test_hps_read",
    "vga_idsp_write_device": "test_idsp_write", "vga_idsp_read_device": "test_idsp_read",
    "vga_adx_write_device": "test_adx_write", "vga_hca_write_device": "test_hca_write",
    "vga_synth_pcm16_device": "test_synth_pcm16",
    # include/vgaudio_hip_pcm.h
    "vga_nwstm_pcm_write_device": "test_nwstm_pcm_write", "vga_nwstm_pcm_read_device": "test_nwstm_pcm_read",
    "vga_pcm8_encode_device": "test_pcm8_encode", "vga_pcm8_decode_device": "test_pcm8_decode",
    "vga_wave_write_pcm8_device": "test_wave_write_pcm8", "vga_wave_deinterleave_pcm8_device": "test_wave_deinterleave_pcm8",
    # include/vgaudio_hip_nwwav.h
    "vga_nwwav_bank_read_device": "test_nwwav_bank_read",
}


def _declared(header):
    """every vga_*_device / vga_*_device_v function `header` declares (the expressions of header_device_entry_points)"""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(vga_\w+_device(?:_v)?)\s*\(", text)) - {"vga_set_device"}


def test_every_pcm_and_nwwav_device_entry_point_has_a_layout_test():
    declared = _declared("vgaudio_hip_pcm.h") | _declared("vgaudio_hip_nwwav.h")
    assert len(declared) >= 7, sorted(declared)
    assert declared <= set(HERE), sorted(declared - set(HERE))
    assert set(HERE) <= declared | _declared("vgaudio_hip.h"), sorted(set(HERE) - declared - _declared("vgaudio_hip.h"))
    own = open(os.path.abspath(__file__)).read()
    for name, test in HERE.items():                              # the named test itself makes the call
        body = _function_body(own, test)
        assert body, (name, test)
        assert re.search(r"\b" + name + r"\(", body), (name, test)


def _granule(*terms):
    """container::pick_granule: the widest of 16, 8, 4, 2, 1 that divides the OR of everything the host was handed"""
    word = 0
    for t in terms:
        word |= int(t)
    return next(g for g in (16, 8, 4, 2, 1) if word % g == 0)


def _last(size, il):
    """the last block of `size` bytes in blocks of `il`"""
    return size - (-(-size // il) - 1) * il if size else 0


def _deinterleave_granule(files, file_pitch, nf, audio_offset, nch, in_, il, dst, dst_pitch):
    """container::deinterleave_images: one channel's single block is a plain copy, and a last block shorter than the
    granule goes byte by byte"""
    several = nch > 1 or -(-in_ // il) > 1
    word = files | (file_pitch if nf > 1 else 0) | audio_offset | (il if several else 0) | dst | dst_pitch
    last = _last(in_, il)
    return next((g for g in (16, 8, 4, 2) if word % g == 0 and (not several or last % g == 0 or last < g)), 1)


def _at(spec, isz=1):
    """(address mod 256, pitch in bytes) of the rows _put(rows, spec, dtype) places: allocations are 256-byte aligned"""
    pitch, off = spec
    pb = pitch * isz
    return ((GUARD + 3 * pb) if off == "view" else off) % 256, pb


# ====================================================================== layout tables
def _byte_rows(nb):
    """rows of nb bytes a container call reads or fills: any byte, any pitch that holds a row"""
    r = _round_up(nb, 16)
    return {"aligned": (r, 0), "base1": (r, 1), "base2": (r, 2), "base4": (r, 4), "base8": (r, 8), "odd_pitch": (nb | 1, 0),
            "min_pitch": (_not_multiple(nb, 8, 16), 0), "both": (nb | 1, "view")}


ROW_LAYOUTS = ["base1", "base2", "base4", "base8", "odd_pitch", "min_pitch"]


def _written_images(size, nf):
    """images a writer fills: any byte; with several, file_pitch a multiple of 16"""
    r = _round_up(size, 16)
    t = {"aligned": (r, 0), "base1": (r, 1), "base2": (r, 2), "base4": (r, 4), "base8": (r, 8), "both": (r + 16, 1)}
    if nf > 1:
        t["pitch16"] = (r + 16, 0)
    return t


def _read_images(size, nf):
    """images a reader takes: any byte, any pitch that holds an image"""
    r = _round_up(size, 16)
    t = {"aligned": (r, 0), "base1": (r, 1), "base2": (r, 2), "base4": (r, 4), "base8": (r, 8), "both": (size | 1, 1)}
    if nf > 1:
        t["odd_pitch"] = (size | 1, 0)
    return t


def _write_layouts(rows, extra=()):
    return (["aligned"] + [f"{rows}:{k}" for k in ROW_LAYOUTS] + [f"files:{k}" for k in ("base1", "base2", "base4", "base8", "pitch16")]
            + list(extra) + ["small", "both"])


def _read_layouts():
    return (["aligned"] + [f"files:{k}" for k in ("base1", "base2", "base4", "base8", "odd_pitch")] + [f"rows:{k}" for k in ROW_LAYOUTS]
            + ["both"])


def _grid(layouts, *axes):
    """the product of axes (the second is nfiles) and layouts, without the file-pitch cases of a single file"""
    out = [()]
    for axis in axes:
        out = [o + (v,) for o in out for v in axis]
    return [o + (lay,) for o in out for lay in layouts if o[1] > 1 or lay not in ("files:pitch16", "files:odd_pitch")]


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _tables(rng, rows, ne=0):
    """seeded coefficients, gains, start and loop contexts (and seek tables of ne entries) for `rows` channels"""
    i16 = lambda *shape: rng.integers(-32768, 32768, shape).astype(np.int16)
    return i16(rows, 16), i16(rows), i16(rows, 3), i16(rows, 3), i16(rows, max(2 * ne, 1))


def _small_tables(tabs, shifted):
    """coefficients, gains and contexts, each one short in when `shifted`"""
    return [small(t, 1 if shifted else 0, np.int16) for t in tabs]


# ====================================================================== BRSTM / BCSTM / BFSTM, GC-ADPCM
NW_TARGETS = [0, 1, 2]                               # VGA_NW_RSTM, CSTM, FSTM
NW_SPE, NW_RATE = 100, 32000
NW_WRITE_CASES = _grid(_write_layouts("adpcm"), [1, 2, 3], [1, 3], [448, 126])
NW_READ_CASES = _grid(_read_layouts(), [1, 2, 3], [1, 3], [448, 126])
# two interleaves and a short block, 72-byte interleave: the padded last block is then 16 bytes, a multiple of 16 where the
# interleave is only one of 8 -- the one geometry in which the interleave alone keeps the granule at 8
NW_WRITE_CASES += [(2, 3, -126, lay) for lay in ("aligned", "adpcm:base8", "both")]
NW_READ_CASES += [(2, 3, -126, lay) for lay in ("aligned", "rows:base8", "both")]


def _nw_n(spi):
    """three interleaves (two for a negative spi) and a last block of 5 samples: 4 bytes unpadded, no multiple of 8"""
    return (3 * spi if spi > 0 else 2 * -spi) + 5


def _nw_geometry(target, nch, spi):
    import nwstm_ref as ref
    n = _nw_n(spi)
    return n, ref.bytes_of(n), ref.layout(target, nch, n, True, 0, n, abs(spi), NW_SPE)


@functools.lru_cache(maxsize=None)
def _nw_case(target, nch, nf, spi):
    """-> (adpcm rows, tables, seek entries per row, the restatement's images)"""
    import nwstm_ref as ref
    from vgaudio_amd import _lib
    n, nb, G = _nw_geometry(target, nch, spi)
    p = _nw_params(target, spi)
    lay = _lib.NwLayoutC()
    _ok(_L().vga_nwstm_layout_for(C.byref(p), nch, C.byref(lay)))
    assert lay.alignment_needed == 0 and lay.channel_adpcm_bytes == nb and lay.channel_seek_entries >= 3
    assert (lay.file_size, lay.audio_data_offset, lay.audio_data_size, lay.interleave_size) == \
        (G["file_size"], G["audio_data_offset"], G["audio_data_size"], G["interleave_size"])
    assert G["interleave_size"] % 16 == (8 if abs(spi) == 126 else 0) and G["last_block_size_without_padding"] % 8 == 4
    ne = lay.channel_seek_entries
    rng = np.random.default_rng(1000 + 100 * target + 10 * nch + nf + abs(spi))
    rows = nf * nch
    adpcm = rng.integers(0, 256, (rows, nb)).astype(np.uint8)
    coefs, gain, sc, lc, seek = _tables(rng, rows, ne)
    images = []
    for f in range(nf):
        r = slice(f * nch, f * nch + nch)
        images.append(np.frombuffer(ref.build_image(target, NW_RATE, nch, [a.tobytes() for a in adpcm[r]], coefs[r].tolist(),
                                                    gain[r].tolist(), sc[r].tolist(), lc[r].tolist(), seek[r].tolist(), True, 0, n, n,
                                                    spi=abs(spi), spe=NW_SPE), np.uint8))
    images = np.stack(images)
    assert images.shape[1] == G["file_size"]
    return _ro(adpcm, coefs, gain, sc, lc, seek, images) + (ne,)


def _nw_params(target, spi):
    from vgaudio_amd import _lib
    p = _lib.NwParamsC()
    n = _nw_n(spi)
    p.target, p.sample_rate, p.sample_count, p.endianness = target, NW_RATE, n, -1
    p.looping, p.loop_start, p.loop_end = 1, 0, n
    p.samples_per_interleave, p.samples_per_seek_table_entry = abs(spi), NW_SPE
    return p


def _nw_write_specs(target, nch, nf, spi, layout):
    n, nb, G = _nw_geometry(target, nch, spi)
    return nb, G, _pick({"adpcm": _byte_rows(nb), "files": _written_images(G["file_size"], nf)}, layout)


def _nw_write_granule(target, nch, nf, spi, layout):
    nb, G, spec = _nw_write_specs(target, nch, nf, spi, layout)
    (sa, sp), (fa, fp) = _at(spec["adpcm"]), _at(spec["files"])
    il = G["interleave_size"]
    return _granule(sa, sp, il, _last(G["audio_data_size"], il), fa + G["audio_data_offset"], fp if nf > 1 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("nch,nf,spi,layout", NW_WRITE_CASES)
def test_nwstm_write(nch, nf, spi, layout):
    """vga_nwstm_write_device, all three targets: looping images (loop start 0) of three interleaves and a 4-byte last
    block, interleaves of 256 and 72 bytes; ADPCM rows and images at any byte, the seek table one short in on an odd
    pitch, coefficients, gains and both contexts one short in"""
    torch = _torch()
    L = _L()
    for target in NW_TARGETS:
        adpcm, coefs, gain, sc, lc, seek, want, ne = _nw_case(target, nch, nf, spi)
        nb, G, spec = _nw_write_specs(target, nch, nf, spi, layout)
        shifted = layout in ("small", "both")
        d_in = _put(adpcm, spec["adpcm"], np.uint8)
        d_files = _put((nf, G["file_size"]), spec["files"], np.uint8)
        d_seek = place(seek, (2 * ne) | 1 if shifted else _round_up(2 * ne, 8), 2 if shifted else 0, np.int16)
        tabs = _small_tables((coefs, gain, sc, lc), shifted)
        p = _nw_params(target, spi)
        _ok(L.vga_nwstm_write_device(C.byref(p), nch, nf, None, d_in.ptr, d_in.pitch, nb, tabs[0].ptr, tabs[1].ptr, tabs[2].ptr,
                                     tabs[3].ptr, d_seek.ptr, d_seek.pitch, ne, d_files.ptr, d_files.pitch, _stream()))
        torch.cuda.synchronize()
        _eq(d_files.rows(), want, f"images (target {target})")
        d_files.kept(f"images (target {target})", padding=True)
        for q, what in [(d_in, "adpcm"), (d_seek, "seek")] + list(zip(tabs, ("coefs", "gain", "start context", "loop context"))):
            q.unchanged(what)


def _nw_read_specs(target, nch, nf, spi, layout):
    n, nb, G = _nw_geometry(target, nch, spi)
    return nb, G, _pick({"files": _read_images(G["file_size"], nf), "rows": _byte_rows(nb)}, layout)


def _nw_read_granule(target, nch, nf, spi, layout):
    nb, G, spec = _nw_read_specs(target, nch, nf, spi, layout)
    (fa, fp), (ra, rp) = _at(spec["files"]), _at(spec["rows"])
    return _deinterleave_granule(fa, fp, nf, G["audio_data_offset"], nch, G["audio_data_size"], G["interleave_size"], ra, rp)


@pytest.mark.gpu
@pytest.mark.parametrize("nch,nf,spi,layout", NW_READ_CASES)
def test_nwstm_read(nch, nf, spi, layout):
    """vga_nwstm_read_device on the restatement's images: images at any byte on any pitch that holds one, rows at any byte
    on any pitch; the rows are what nwstm_ref.parse_image and gc_containers_ref.deinterleave take out of each image"""
    import gc_containers_ref as gref
    import nwstm_ref as ref
    from vgaudio_amd.nwstm import parse
    torch = _torch()
    for target in NW_TARGETS:
        adpcm, _, _, _, _, _, images, _ = _nw_case(target, nch, nf, spi)
        nb, G, spec = _nw_read_specs(target, nch, nf, spi, layout)
        info = parse(images[0].tobytes())
        assert (info.adpcm_bytes, info.channel_count, info.audio_data_offset, info.interleave_size) == \
            (nb, nch, G["audio_data_offset"], G["interleave_size"])
        want = []
        for f in range(nf):
            R = ref.parse_image(images[f].tobytes())
            rows = gref.deinterleave(images[f][R["audio_offset"]:].tobytes(), R["audio_length"], R["interleave_size"], nch, nb)
            assert rows == R["audio"]
            want += [np.frombuffer(r, np.uint8) for r in rows]
        want = np.stack(want)
        assert np.array_equal(want, adpcm)
        d_files = _put(list(images), spec["files"], np.uint8)
        d_rows = _put((nf * nch, nb), spec["rows"], np.uint8)
        _ok(_L().vga_nwstm_read_device(C.byref(info), d_files.ptr, d_files.pitch, nf, d_rows.ptr, d_rows.pitch, _stream()))
        torch.cuda.synchronize()
        _eq(d_rows.rows(), want, f"rows (target {target})")
        d_rows.kept(f"rows (target {target})", padding=True)
        d_files.unchanged("images")


# ====================================================================== IDSP
IDSP_N, IDSP_LOOP_END, IDSP_RATE = 14 * 300 + 5, 14 * 300 + 5 - 100, 44100
IDSP_BLOCKS = [0, 0x10, 0x38]
IDSP_WRITE_CASES = _grid(_write_layouts("adpcm"), [1, 3], [1, 3], IDSP_BLOCKS)
IDSP_READ_CASES = _grid(_read_layouts(), [1, 3], [1, 3], IDSP_BLOCKS)


def _idsp_geometry(nch, block, trim):
    import gc_containers_ref as ref
    return ref.bytes_of(IDSP_N), ref.idsp_layout(nch, IDSP_N, True, 0, IDSP_LOOP_END, block, bool(trim))


def _idsp_params(block, trim):
    from vgaudio_amd import _lib
    return _lib.IdspParamsC(IDSP_RATE, IDSP_N, 1, 0, IDSP_LOOP_END, block, trim)


@functools.lru_cache(maxsize=None)
def _idsp_case(nch, nf, block, trim):
    """a looping file (loop start 0) whose loop ends 100 samples early: trimmed, the rows are longer than the image holds"""
    import gc_containers_ref as ref
    from vgaudio_amd import _lib
    nb, G = _idsp_geometry(nch, block, trim)
    p = _idsp_params(block, trim)
    lay = _lib.IdspLayoutC()
    _ok(_L().vga_idsp_layout_for(C.byref(p), nch, C.byref(lay)))
    assert lay.alignment_needed == 0 and lay.channel_adpcm_bytes == nb
    assert (lay.file_size, lay.header_size, lay.audio_data_size, lay.interleave_size) == \
        (G["file_size"], G["header_size"], G["audio_data_size"], G["interleave"])
    rng = np.random.default_rng(2000 + 100 * block + 10 * nch + 2 * nf + trim)
    rows = nf * nch
    adpcm = rng.integers(0, 256, (rows, nb)).astype(np.uint8)
    coefs, gain, sc, lc, _ = _tables(rng, rows)
    images = []
    for f in range(nf):
        r = slice(f * nch, f * nch + nch)
        images.append(np.frombuffer(ref.idsp_image(IDSP_RATE, [a.tobytes() for a in adpcm[r]], coefs[r].tolist(), gain[r].tolist(),
                                                   sc[r].tolist(), lc[r].tolist(), True, 0, IDSP_LOOP_END, IDSP_N, block, bool(trim)),
                                    np.uint8))
    return _ro(adpcm, coefs, gain, sc, lc, np.stack(images))


def _idsp_write_specs(nch, nf, block, trim, layout):
    nb, G = _idsp_geometry(nch, block, trim)
    return nb, G, _pick({"adpcm": _byte_rows(nb), "files": _written_images(G["file_size"], nf)}, layout)


def _idsp_write_granule(nch, nf, block, trim, layout):
    nb, G, spec = _idsp_write_specs(nch, nf, block, trim, layout)
    (sa, sp), (fa, fp) = _at(spec["adpcm"]), _at(spec["files"])
    il = G["interleave"]
    return _granule(sa, sp, il, _last(G["audio_data_size"], il), fa + G["header_size"], fp if nf > 1 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("nch,nf,block,layout", IDSP_WRITE_CASES)
def test_idsp_write(nch, nf, block, layout):
    """vga_idsp_write_device, trimmed and not: not interleaved (one block of the whole channel), 16- and 56-byte blocks"""
    torch = _torch()
    for trim in (0, 1):
        adpcm, coefs, gain, sc, lc, want = _idsp_case(nch, nf, block, trim)
        nb, G, spec = _idsp_write_specs(nch, nf, block, trim, layout)
        d_in = _put(adpcm, spec["adpcm"], np.uint8)
        d_files = _put((nf, G["file_size"]), spec["files"], np.uint8)
        tabs = _small_tables((coefs, gain, sc, lc), layout in ("small", "both"))
        p = _idsp_params(block, trim)
        _ok(_L().vga_idsp_write_device(C.byref(p), nch, nf, d_in.ptr, d_in.pitch, nb, tabs[0].ptr, tabs[1].ptr, tabs[2].ptr, tabs[3].ptr,
                                       d_files.ptr, d_files.pitch, _stream()))
        torch.cuda.synchronize()
        _eq(d_files.rows(), want, f"images (trim {trim})")
        d_files.kept(f"images (trim {trim})", padding=True)
        for q, what in [(d_in, "adpcm")] + list(zip(tabs, ("coefs", "gain", "start context", "loop context"))):
            q.unchanged(what)


def _idsp_read_specs(nch, nf, block, trim, layout):
    import gc_containers_ref as ref
    nb, G = _idsp_geometry(nch, block, trim)
    ab = ref.bytes_of(G["sample_count"])
    return ab, G, _pick({"files": _read_images(G["file_size"], nf), "rows": _byte_rows(ab)}, layout)


def _idsp_read_granule(nch, nf, block, trim, layout):
    ab, G, spec = _idsp_read_specs(nch, nf, block, trim, layout)
    (fa, fp), (ra, rp) = _at(spec["files"]), _at(spec["rows"])
    return _deinterleave_granule(fa, fp, nf, G["header_size"], nch, G["audio_data_size"], G["interleave"], ra, rp)


@pytest.mark.gpu
@pytest.mark.parametrize("nch,nf,block,layout", IDSP_READ_CASES)
def test_idsp_read(nch, nf, block, layout):
    """vga_idsp_read_device on the restatement's images; the rows are gc_containers_ref.idsp_parse's"""
    import gc_containers_ref as ref
    from vgaudio_amd.idsp import parse
    torch = _torch()
    for trim in (0, 1):
        adpcm, _, _, _, _, images = _idsp_case(nch, nf, block, trim)
        ab, G, spec = _idsp_read_specs(nch, nf, block, trim, layout)
        info = parse(images[0].tobytes())
        assert (info.adpcm_bytes, info.channel_count, info.audio_data_offset, info.interleave) == (ab, nch, G["header_size"], G["interleave"])
        want = np.stack([np.frombuffer(r, np.uint8) for f in range(nf) for r in ref.idsp_parse(images[f].tobytes())["audio"]])
        assert np.array_equal(want, adpcm[:, :ab])
        d_files = _put(list(images), spec["files"], np.uint8)
        d_rows = _put((nf * nch, ab), spec["rows"], np.uint8)
        _ok(_L().vga_idsp_read_device(C.byref(info), d_files.ptr, d_files.pitch, nf, d_rows.ptr, d_rows.pitch, _stream()))
        torch.cuda.synchronize()
        _eq(d_rows.rows(), want, f"rows (trim {trim})")
        d_rows.kept(f"rows (trim {trim})", padding=True)
        d_files.unchanged("images")


# ====================================================================== HPS
HPS_RATE = 32000
HPS_SHAPES = [(1, False), (2, False), (8, False), (8, True)]          # (channels, looping); 3 and 7 channels are refused by design
HPS_WRITE_CASES = [(nch, nf, loop, lay) for nch, loop in HPS_SHAPES for nf in (1, 3) for lay in _write_layouts("adpcm", extra=["pcm:odd"])
                   if nf > 1 or lay != "files:pitch16"]
HPS_READ_CASES = [(nch, nf, loop, lay) for nch, loop in HPS_SHAPES for nf in (1, 3) for lay in _read_layouts()
                  if nf > 1 or lay != "files:odd_pitch"]


def _hps_geometry(nch, loop):
    """two full blocks and a partial one: byte_in_index, a second block header and a short channel_size all occur"""
    import gc_containers_ref as ref
    alignment = ref.byte_count_to_sample_count(ref.next_multiple(0x10000 // nch, 0x20))
    n = 2 * alignment + 777
    G = ref.hps_layout(nch, n, loop, alignment if loop else 0, n if loop else 0)
    assert G["alignment"] == alignment and len(G["blocks"]) == 3 and G["blocks"][1]["byte_in_index"] > 0
    assert G["blocks"][2]["channel_size"] < G["blocks"][0]["channel_size"] and G["sample_count"] == n
    return n, alignment, ref.bytes_of(n), G


def _hps_params(nch, loop):
    from vgaudio_amd import _lib
    n, alignment, _, _ = _hps_geometry(nch, loop)
    return _lib.HpsParamsC(HPS_RATE, n, int(loop), alignment if loop else 0, n if loop else 0)


@functools.lru_cache(maxsize=None)
def _hps_case(nch, nf, loop):
    import gc_containers_ref as ref
    from vgaudio_amd import _lib
    n, alignment, nb, G = _hps_geometry(nch, loop)
    p = _hps_params(nch, loop)
    lay = _lib.HpsLayoutC()
    _ok(_L().vga_hps_layout_for(C.byref(p), nch, C.byref(lay)))
    assert lay.alignment_needed == 0 and lay.channel_adpcm_bytes == nb and lay.block_count == 3
    assert (lay.file_size, lay.header_size, lay.block_header_size) == (G["file_size"], G["header_size"], ref.next_multiple(12 + 8 * nch, 0x20))
    rng = np.random.default_rng(3000 + 10 * nch + 2 * nf + loop)
    rows = nf * nch
    adpcm = rng.integers(0, 256, (rows, nb)).astype(np.uint8)
    pcm = rng.integers(-32768, 32768, (rows, n)).astype(np.int16)
    coefs, gain, sc, _, _ = _tables(rng, rows)
    images = []
    for f in range(nf):
        r = slice(f * nch, f * nch + nch)
        images.append(np.frombuffer(ref.hps_image(HPS_RATE, [a.tobytes() for a in adpcm[r]], coefs[r].tolist(), gain[r].tolist(),
                                                  sc[r].tolist(), list(pcm[r]), loop, alignment if loop else 0, n if loop else 0, n),
                                    np.uint8))
    return _ro(adpcm, pcm, coefs, gain, sc, np.stack(images))


def _hps_pcm(n):
    return {"aligned": (_round_up(n, 8), 0), "odd": (n | 1, 2), "both": (n | 1, 2)}


def _hps_write_specs(nch, nf, loop, layout):
    n, _, nb, G = _hps_geometry(nch, loop)
    return n, nb, G, _pick({"adpcm": _byte_rows(nb), "files": _written_images(G["file_size"], nf), "pcm": _hps_pcm(n)}, layout)


def _hps_write_granule(nch, nf, loop, layout):
    import gc_containers_ref as ref
    n, nb, G, spec = _hps_write_specs(nch, nf, loop, layout)
    (sa, sp), (fa, fp) = _at(spec["adpcm"]), _at(spec["files"])
    return _granule(sa, sp, fa, fp if nf > 1 else 0, G["header_size"], ref.next_multiple(12 + 8 * nch, 0x20))


@pytest.mark.gpu
@pytest.mark.parametrize("nch,nf,loop,layout", HPS_WRITE_CASES)
def test_hps_write(nch, nf, loop, layout):
    """vga_hps_write_device: three blocks, the PCM rows behind the block headers' histories one sample in on an odd
    pitch; with 8 channels also a file that loops from the second block"""
    torch = _torch()
    adpcm, pcm, coefs, gain, sc, want = _hps_case(nch, nf, loop)
    n, nb, G, spec = _hps_write_specs(nch, nf, loop, layout)
    d_in = _put(adpcm, spec["adpcm"], np.uint8)
    d_pcm = _put(pcm, spec["pcm"], np.int16)
    d_files = _put((nf, G["file_size"]), spec["files"], np.uint8)
    tabs = _small_tables((coefs, gain, sc), layout in ("small", "both"))
    p = _hps_params(nch, loop)
    _ok(_L().vga_hps_write_device(C.byref(p), nch, nf, d_in.ptr, d_in.pitch, nb, tabs[0].ptr, tabs[1].ptr, tabs[2].ptr, d_pcm.ptr,
                                  d_pcm.pitch, n, d_files.ptr, d_files.pitch, _stream()))
    torch.cuda.synchronize()
    _eq(d_files.rows(), want, "images")
    d_files.kept("images", padding=True)
    for q, what in [(d_in, "adpcm"), (d_pcm, "pcm")] + list(zip(tabs, ("coefs", "gain", "start context"))):
        q.unchanged(what)


def _hps_read_specs(nch, nf, loop, layout):
    n, _, nb, G = _hps_geometry(nch, loop)
    return nb, G, _pick({"files": _read_images(G["file_size"], nf), "rows": _byte_rows(nb)}, layout)


def _hps_read_granule(nch, nf, loop, layout):
    import gc_containers_ref as ref
    nb, G, spec = _hps_read_specs(nch, nf, loop, layout)
    (fa, fp), (ra, rp) = _at(spec["files"]), _at(spec["rows"])
    terms, out = [fa, fp if nf > 1 else 0, ra, rp], 0
    for B in G["blocks"]:                                         # audio offset, channel stride and where the block lands
        terms += [B["offset"] + ref.next_multiple(12 + 8 * nch, 0x20), B["written_size"] // nch, out]
        out += B["channel_size"]
    return _granule(*terms)


@pytest.mark.gpu
@pytest.mark.parametrize("nch,nf,loop,layout", HPS_READ_CASES)
def test_hps_read(nch, nf, loop, layout):
    """vga_hps_read_device on the restatement's images; the rows are gc_containers_ref.hps_parse's"""
    import gc_containers_ref as ref
    from vgaudio_amd.hps import parse
    torch = _torch()
    adpcm, _, _, _, _, images = _hps_case(nch, nf, loop)
    nb, G, spec = _hps_read_specs(nch, nf, loop, layout)
    info, blocks = parse(images[0].tobytes())
    assert info.channel_count == nch and info.block_count == 3
    assert info.adpcm_bytes == nb                                # the blocks' audio adds up to the channel
    want = np.stack([np.frombuffer(r, np.uint8) for f in range(nf) for r in ref.hps_parse(images[f].tobytes())["audio"]])
    assert np.array_equal(want, adpcm)
    d_files = _put(list(images), spec["files"], np.uint8)
    d_rows = _put((nf * nch, nb), spec["rows"], np.uint8)
    _ok(_L().vga_hps_read_device(C.byref(info), blocks, d_files.ptr, d_files.pitch, nf, d_rows.ptr, d_rows.pitch, _stream()))
    torch.cuda.synchronize()
    _eq(d_rows.rows(), want, "rows")
    d_rows.kept("rows", padding=True)
    d_files.unchanged("images")


# ====================================================================== ADX
# (version, channels, frame size, frames the rows are short of frame_count * frame_size)
ADX_SHAPES = ([(v, nch, 18, 0) for v in (3, 4) for nch in (1, 2, 5)]
              + [(4, 2, 34, 0), (4, 1, 18, 1), (4, 2, 18, 1)])           # 34-byte frames; the zero gap on both paths
ADX_LAYOUTS = ["aligned", "audio:odd", "audio:base2", "history", "file:base1", "file:base2", "file:base4", "file:base8", "both"]
ADX_WRITE_CASES = [s + (lay,) for s in ADX_SHAPES for lay in ADX_LAYOUTS]
ADX_RATE = 48000


def _adx_geometry(version, nch, fs, short):
    spf = (fs - 2) * 2
    n = spf * 300 + 13                                           # 300 frames and a partial one
    frames = -(-n // spf)
    header = 36 if version == 4 else 32
    return n, (frames - short) * fs, dict(audio_offset=header + 4, file_size=header + 4 + fs * frames * nch + fs, frames=frames)


def _adx_specs(version, nch, fs, short, layout):
    n, nb, G = _adx_geometry(version, nch, fs, short)
    r = _round_up(nb, 16)
    audio = {"aligned": (r, 0), "odd": (nb | 1, 1), "base2": (r, 2), "both": (nb | 1, "view")}
    size = G["file_size"]
    file = {"aligned": (size, 0), "base1": (size, 1), "base2": (size, 2), "base4": (size, 4), "base8": (size, 8), "both": (size, 1)}
    return n, nb, G, _pick({"audio": audio, "file": file}, layout)


def _adx_write_granule(version, nch, fs, short, layout):
    """container::launch_interleave: one channel is a plain copy in one block (the interleave drops out of the word)"""
    n, nb, G, spec = _adx_specs(version, nch, fs, short, layout)
    (sa, sp), (fa, _) = _at(spec["audio"]), _at(spec["file"])
    return _granule(sa, fa + G["audio_offset"], sp, *((fs, fs) if nch > 1 else ()))


@functools.lru_cache(maxsize=None)
def _adx_case(version, nch, fs, short):
    from oracle.pyref import containers as rcont
    n, nb, G = _adx_geometry(version, nch, fs, short)
    rng = np.random.default_rng(4000 + 100 * version + 10 * nch + fs + short)
    audio = rng.integers(0, 256, (nch, nb)).astype(np.uint8)
    hist = rng.integers(-32768, 32768, nch).astype(np.int16)
    want = np.frombuffer(rcont.adx_write([a.tobytes() for a in audio], hist.tolist(), ADX_RATE, n, frame_size=fs, version=version),
                         np.uint8)
    assert len(want) == G["file_size"]
    return _ro(audio, hist, want)


@pytest.mark.gpu
@pytest.mark.parametrize("version,nch,fs,short,layout", ADX_WRITE_CASES)
def test_adx_write(version, nch, fs, short, layout):
    """vga_adx_write_device, versions 3 and 4 (whose header carries d_history): one channel is the plain-copy path that
    may take 16-byte granules over a length that is no multiple of 16, several interleave 18- (34-)byte frames with a
    granule of 2 at most; rows a frame short leave the zero gap"""
    from vgaudio_amd import _lib
    torch = _torch()
    audio, hist, want = _adx_case(version, nch, fs, short)
    n, nb, G, spec = _adx_specs(version, nch, fs, short, layout)
    p = _lib.AdxFileParamsC(ADX_RATE, n, 0, 0, 0, 0, fs, version, 3, 500, 0, 1)
    lay = _lib.AdxFileLayoutC()
    _ok(_L().vga_adx_file_layout_for(C.byref(p), nch, C.byref(lay)))
    assert (lay.file_size, lay.audio_offset, lay.frame_count) == (G["file_size"], G["audio_offset"], G["frames"])
    d_in = _put(audio, spec["audio"], np.uint8)
    d_hist = small(hist, 1 if layout in ("history", "both") else 0, np.int16)
    d_file = _put((1, G["file_size"]), spec["file"], np.uint8)
    _ok(_L().vga_adx_write_device(d_in.ptr, d_in.pitch, nb, d_hist.ptr, nch, C.byref(p), d_file.ptr, _stream()))
    torch.cuda.synchronize()
    _eq(d_file.rows()[0], want, "image")
    d_file.kept("image", padding=True)
    d_in.unchanged("audio")
    d_hist.unchanged("history")


# ====================================================================== HCA
HCA_NS, HCA_N = 3, 1024 * 20
HCA_WRITE_CASES = ["aligned", "frames:odd", "files:odd", "both"]


@functools.lru_cache(maxsize=None)
def _hca_case(comment):
    from oracle import pyoracle as po
    from oracle.pyref import containers as rcont
    from vgaudio_amd import _lib
    cfg = _lib.HcaParamsC(po.HCA_QUALITY["High"], 0, 0, 2, 48000, HCA_N, 0, 0, 0)
    info = _lib.HcaInfoC()
    _ok(_L().vga_hca_encoder_initialize(C.byref(cfg), C.byref(info)))
    assert 20 <= info.frame_count <= 24
    if comment:                                                  # the encoder sizes the header for the comment it is given
        info.comment_length = len(comment.encode())
        info.header_size = _round_up(96 + info.comment_length + 1, 32)
    audio = info.frame_size * info.frame_count
    frames = np.random.default_rng(5000 + len(comment or "")).integers(0, 256, (HCA_NS, audio)).astype(np.uint8)
    want = np.stack([np.frombuffer(rcont.hca_write(info, [frames[s, k * info.frame_size:(k + 1) * info.frame_size].tobytes()
                                                          for k in range(info.frame_count)], comment=comment), np.uint8)
                     for s in range(HCA_NS)])
    return (info,) + _ro(frames, want)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", HCA_WRITE_CASES)
@pytest.mark.parametrize("comment", [None, "a comment of some length"])
def test_hca_write(comment, layout):
    """vga_hca_write_device, three streams of about 20 frames: frames and images at odd bases on odd pitches (this call has
    no multiple-of-16 rule: the header goes byte by byte and the frames as a 2-D copy)"""
    torch = _torch()
    info, frames, want = _hca_case(comment)
    audio, size = frames.shape[1], want.shape[1]
    assert _L().vga_hca_file_size(C.byref(info)) == size
    fr = (audio | 1, 1) if layout in ("frames:odd", "both") else (_round_up(audio, 16), 0)
    fl = (size | 1, 1) if layout in ("files:odd", "both") else (_round_up(size, 16), 0)
    d_in = _put(frames, fr, np.uint8)
    d_files = _put((HCA_NS, size), fl, np.uint8)
    _ok(_L().vga_hca_write_device(C.byref(info), d_in.ptr, d_in.pitch, HCA_NS, comment.encode() if comment else None, 1.0, 0, 0,
                                  d_files.ptr, d_files.pitch, _stream()))
    torch.cuda.synchronize()
    _eq(d_files.rows(), want, "images")
    d_files.kept("images", padding=True)
    d_in.unchanged("frames")


# ====================================================================== synthetic PCM
@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["aligned", "odd"])
def test_synth_pcm16(layout):
    """vga_synth_pcm16_device: five channels from channel 7 on, rows one sample in on an odd pitch, the parameters one
    uint32 in"""
    from vgaudio_amd import synth
    torch = _torch()
    nch, n, first = 5, 1000 + 3, 7
    want = synth.generate(nch, n, first_channel=first)
    params = np.array([synth.channel_params(first + c) for c in range(nch)], dtype=np.uint32)
    odd = layout == "odd"
    d_params = small(params, 1 if odd else 0, np.uint32)
    d_pcm = place((nch, n), n | 1 if odd else _round_up(n, 8), 2 if odd else 0, np.int16)
    _ok(_L().vga_synth_pcm16_device(d_pcm.ptr, d_pcm.pitch, nch, n, first, d_params.ptr, _stream()))
    torch.cuda.synchronize()
    _eq(d_pcm.rows(), np.asarray(want, dtype=np.int16), "pcm")
    d_pcm.kept("pcm", padding=True)
    d_params.unchanged("params")


# ====================================================================== BRSTM / BCSTM / BFSTM, PCM8 and PCM16
# the shapes of test_gpu_nwstm_pcm.py::test_every_granule_size: (codec, sample kind, big-endian)
PCM_KINDS = [(PCM16, S16, True), (PCM16, S16, False), (PCM8, S16, True), (PCM8, BYTES, True)]
PCM_SPI = [255, 256, 258]
PCM_NCH, PCM_NF, PCM_N, PCM_RATE = 3, 3, 2003, 48000
PCM_ROW_LAYOUTS = ["base1", "base2", "base4", "base8", "odd_pitch"]
PCM_WRITE_LAYOUTS = (["aligned"] + [f"rows:{k}" for k in PCM_ROW_LAYOUTS] + [f"files:{k}" for k in ("base1", "base2", "base4", "base8", "pitch16")]
                     + ["both"])
PCM_READ_LAYOUTS = (["aligned"] + [f"files:{k}" for k in ("base1", "base2", "base4", "base8", "odd_pitch")] + [f"rows:{k}" for k in PCM_ROW_LAYOUTS]
                    + ["both"])
PCM_WRITE_CASES = [(k, spi, lay) for k in range(len(PCM_KINDS)) for spi in PCM_SPI for lay in PCM_WRITE_LAYOUTS]
PCM_READ_CASES = [(k, spi, lay) for k in range(len(PCM_KINDS)) for spi in PCM_SPI for lay in PCM_READ_LAYOUTS]


def _pcm_rows(es):
    """sample rows (es bytes per element): any element boundary, any pitch that holds a row; baseK is K ELEMENTS in"""
    r = _round_up(PCM_N, 16)
    return {"aligned": (r, 0), "base1": (r, es), "base2": (r, 2 * es), "base4": (r, 4 * es), "base8": (r, 8 * es),
            "odd_pitch": (PCM_N | 1, 0), "both": (PCM_N | 1, "view")}


def _pcm_geometry(k, spi):
    import nwstm_pcm_ref as ref
    codec, kind, big = PCM_KINDS[k]
    return ref.layout(ref.FSTM, codec, PCM_NCH, PCM_N, spi=spi)


def _pcm_params(k, spi):
    from vgaudio_amd import _lib
    p = _lib.NwParamsC()
    p.target, p.sample_rate, p.sample_count, p.endianness = 2, PCM_RATE, PCM_N, int(PCM_KINDS[k][2])
    p.samples_per_interleave = spi
    return p


@functools.lru_cache(maxsize=None)
def _pcm_case(k, spi):
    """-> (rows as handed over, rows as read back, the restatement's images)"""
    import nwstm_pcm_ref as ref
    from vgaudio_amd import _lib
    codec, kind, big = PCM_KINDS[k]
    G = _pcm_geometry(k, spi)
    lay = _lib.NwLayoutC()
    p = _pcm_params(k, spi)
    _ok(_L().vga_nwstm_pcm_layout_for(C.byref(p), codec, PCM_NCH, C.byref(lay)))
    assert (lay.file_size, lay.audio_data_offset, lay.audio_data_size, lay.interleave_size) == \
        (G["file_size"], G["audio_data_offset"], G["audio_data_size"], G["interleave_size"])
    rng = np.random.default_rng(6000 + 10 * k + spi)
    shape = (PCM_NF * PCM_NCH, PCM_N)
    rows = (rng.integers(-32768, 32768, shape).astype(np.int16) if kind == S16 else rng.integers(0, 256, shape).astype(np.uint8))
    stored = ref.encode_signed(rows) if (codec == PCM8 and kind == S16) else rows
    back = ref.decode_signed(stored) if (codec == PCM8 and kind == S16) else rows
    images = np.stack([np.frombuffer(ref.build_image(ref.FSTM, codec, PCM_RATE, list(stored[f * PCM_NCH:(f + 1) * PCM_NCH]), spi=spi, big=big),
                                     np.uint8) for f in range(PCM_NF)])
    return _ro(rows, back, images)


def _pcm_specs(k, spi, layout, write):
    codec, kind, big = PCM_KINDS[k]
    es = 2 if kind == S16 else 1
    G = _pcm_geometry(k, spi)
    images = _written_images(G["file_size"], PCM_NF) if write else _read_images(G["file_size"], PCM_NF)
    return es, G, _pick({"rows": _pcm_rows(es), "files": images}, layout)


def _pcm_plain(k):
    """the rows' bytes are the file's: container::interleave_images / deinterleave_images, else the pcm:: kernels"""
    codec, kind, big = PCM_KINDS[k]
    return kind == BYTES or (codec == PCM16 and not big)


def _pcm_write_granule(k, spi, layout):
    es, G, spec = _pcm_specs(k, spi, layout, True)
    (ra, rp), (fa, fp) = _at(spec["rows"], es), _at(spec["files"])
    il = G["interleave_size"]
    out = [fa + G["audio_data_offset"], fp, il, _last(G["audio_data_size"], il)]
    if _pcm_plain(k) or PCM_KINDS[k][0] == PCM16:                # in bytes of the rows
        return _granule(ra, rp, *out)
    return _granule(ra >> 1, rp >> 1, *out)                      # PCM8 from int16 rows: a granule reads G samples


def _pcm_read_granule(k, spi, layout):
    es, G, spec = _pcm_specs(k, spi, layout, False)
    (ra, rp), (fa, fp) = _at(spec["rows"], es), _at(spec["files"])
    il, in_ = G["interleave_size"], G["audio_data_size"]
    if _pcm_plain(k):
        return _deinterleave_granule(fa, fp, PCM_NF, G["audio_data_offset"], PCM_NCH, in_, il, ra, rp)
    src = [fa, fp, G["audio_data_offset"], il, _last(in_, il)]
    return _granule(*src, ra, rp) if PCM_KINDS[k][0] == PCM16 else _granule(*src, ra >> 1, rp >> 1)


@pytest.mark.gpu
@pytest.mark.parametrize("k,spi,layout", PCM_WRITE_CASES)
def test_nwstm_pcm_write(k, spi, layout):
    """vga_nwstm_pcm_write_device, three BFSTM images of three channels: PCM16 big- and little-endian, PCM8 from int16 rows
    and from byte rows; interleaves of 255, 256 and 258 samples; rows as a view of a larger batch in `both`"""
    torch = _torch()
    codec, kind, big = PCM_KINDS[k]
    rows, _, want = _pcm_case(k, spi)
    es, G, spec = _pcm_specs(k, spi, layout, True)
    d_in = _put(rows, spec["rows"], rows.dtype)
    d_files = _put((PCM_NF, G["file_size"]), spec["files"], np.uint8)
    p = _pcm_params(k, spi)
    _ok(_L().vga_nwstm_pcm_write_device(C.byref(p), codec, PCM_NCH, PCM_NF, None, d_in.ptr, kind, d_in.pitch, d_files.ptr, d_files.pitch,
                                        _stream()))
    torch.cuda.synchronize()
    _eq(d_files.rows(), want, "images")
    d_files.kept("images", padding=True)
    d_in.unchanged("rows")


@pytest.mark.gpu
@pytest.mark.parametrize("k,spi,layout", PCM_READ_CASES)
def test_nwstm_pcm_read(k, spi, layout):
    """vga_nwstm_pcm_read_device on the restatement's images, the same kinds and interleaves; the rows are
    nwstm_pcm_ref.parse_image's channels (through DecodeSigned for PCM8 into int16 rows)"""
    import nwstm_pcm_ref as ref
    from vgaudio_amd.nwstm import parse_pcm
    torch = _torch()
    codec, kind, big = PCM_KINDS[k]
    rows, want, images = _pcm_case(k, spi)
    es, G, spec = _pcm_specs(k, spi, layout, False)
    info = parse_pcm(images[0].tobytes())
    assert (info.sample_count, info.channel_count, info.audio_data_offset, info.interleave_size) == \
        (PCM_N, PCM_NCH, G["audio_data_offset"], G["interleave_size"])
    for f in range(PCM_NF):
        for c, ch in enumerate(ref.parse_image(images[f].tobytes())["channels"]):
            stored = np.asarray(ch)
            assert np.array_equal(ref.decode_signed(stored) if (codec == PCM8 and kind == S16) else stored, want[f * PCM_NCH + c])
    d_files = _put(list(images), spec["files"], np.uint8)
    d_rows = _put((PCM_NF * PCM_NCH, PCM_N), spec["rows"], rows.dtype)
    _ok(_L().vga_nwstm_pcm_read_device(C.byref(info), d_files.ptr, d_files.pitch, PCM_NF, d_rows.ptr, kind, d_rows.pitch, _stream()))
    torch.cuda.synchronize()
    _eq(d_rows.rows(), want, "rows")
    d_rows.kept("rows", padding=True)
    d_files.unchanged("images")


# ====================================================================== Pcm8Codec
P8_ROWS, P8_N = 5, 1000 + 3


def _p8_layout(layout, isz):
    """(pitch, base offset in bytes): the control, or one element in on an odd pitch"""
    return ((P8_N | 1) + 2, isz) if layout == "odd" else (_round_up(P8_N, 16), 0)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["aligned", "odd"])
@pytest.mark.parametrize("signed", [0, 1])
def test_pcm8_encode(signed, layout):
    """vga_pcm8_encode_device against the header's formulas: (s + 0x8000) >> 8 and s >> 8"""
    torch = _torch()
    pcm = np.random.default_rng(70 + signed).integers(-32768, 32768, (P8_ROWS, P8_N)).astype(np.int16)
    pcm[0, :4] = (-32768, 32767, -1, 0)
    s = pcm.astype(np.int32)
    want = ((s >> 8) if signed else ((s + 0x8000) >> 8)).astype(np.uint8)
    d_in = place(pcm, *_p8_layout(layout, 2), np.int16)
    d_out = place((P8_ROWS, P8_N), *_p8_layout(layout, 1), np.uint8)
    _ok(_L().vga_pcm8_encode_device(d_in.ptr, d_in.pitch, P8_N, P8_ROWS, signed, d_out.ptr, d_out.pitch, _stream()))
    torch.cuda.synchronize()
    _eq(d_out.rows(), want, "bytes")
    d_out.kept("bytes", padding=True)
    d_in.unchanged("pcm")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["aligned", "odd"])
@pytest.mark.parametrize("signed", [0, 1])
def test_pcm8_decode(signed, layout):
    """vga_pcm8_decode_device against the header's formulas: (b - 0x80) << 8 and (sbyte)b << 8"""
    torch = _torch()
    data = np.random.default_rng(72 + signed).integers(0, 256, (P8_ROWS, P8_N)).astype(np.uint8)
    data[0, :4] = (0, 0x7f, 0x80, 0xff)
    b = data.astype(np.int32)
    want = (((b ^ 0x80) - 0x80) * 256 if signed else (b - 0x80) * 256).astype(np.int16)
    d_in = place(data, *_p8_layout(layout, 1), np.uint8)
    d_out = place((P8_ROWS, P8_N), *_p8_layout(layout, 2), np.int16)
    _ok(_L().vga_pcm8_decode_device(d_in.ptr, d_in.pitch, P8_N, P8_ROWS, signed, d_out.ptr, d_out.pitch, _stream()))
    torch.cuda.synchronize()
    _eq(d_out.rows(), want, "pcm")
    d_out.kept("pcm", padding=True)
    d_in.unchanged("bytes")


# ====================================================================== WAVE, 8-bit
WAVE_N, WAVE_RATE = 1001, 22050
WAVE_LAYOUTS = ["aligned", "file:base1", "file:base3", "rows:odd", "both"]


@functools.lru_cache(maxsize=None)
def _wave_case(nch, kind):
    """-> (rows as handed over, rows as read back, the image test_gpu_wave_pcm8.py holds the writer to)"""
    import test_gpu_wave_pcm8 as w8
    rng = np.random.default_rng(80 + nch + kind)
    if kind == S16:
        rows = rng.integers(-32768, 32768, (nch, WAVE_N)).astype(np.int16)
        stored = w8.encode(rows)
        back = w8.decode(stored)
    else:
        rows = stored = back = rng.integers(0, 256, (nch, WAVE_N)).astype(np.uint8)
    image = np.frombuffer(w8.wave8(list(stored), WAVE_RATE), np.uint8)
    return _ro(rows, back, image.copy())


def _wave_specs(layout, size, es):
    rows = ((WAVE_N | 1) + 2, es) if layout in ("rows:odd", "both") else (_round_up(WAVE_N, 16), 0)
    off = {"file:base1": 1, "file:base3": 3, "both": 3}.get(layout, 0)
    return rows, (size, off)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", WAVE_LAYOUTS)
@pytest.mark.parametrize("kind", [S16, BYTES])
@pytest.mark.parametrize("nch", [1, 2, 5])
def test_wave_write_pcm8(nch, kind, layout):
    """vga_wave_write_pcm8_device, an odd sample count: the image 1 and 3 bytes in, rows one element in on an odd pitch"""
    from vgaudio_amd import _lib
    torch = _torch()
    rows, _, want = _wave_case(nch, kind)
    p = _lib.WaveParamsC(WAVE_RATE, WAVE_N, 0, 0, 0)
    assert _L().vga_wave_pcm8_file_size(C.byref(p), nch) == len(want)
    rspec, fspec = _wave_specs(layout, len(want), rows.dtype.itemsize)
    d_in = _put(rows, rspec, rows.dtype)
    d_file = _put((1, len(want)), fspec, np.uint8)
    _ok(_L().vga_wave_write_pcm8_device(d_in.ptr, kind, d_in.pitch, nch, C.byref(p), d_file.ptr, _stream()))
    torch.cuda.synchronize()
    _eq(d_file.rows()[0], want, "image")
    d_file.kept("image", padding=True)
    d_in.unchanged("rows")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", WAVE_LAYOUTS)
@pytest.mark.parametrize("kind", [S16, BYTES])
@pytest.mark.parametrize("nch", [1, 2, 5])
def test_wave_deinterleave_pcm8(nch, kind, layout):
    """vga_wave_deinterleave_pcm8_device: the data chunk of the same image 1 and 3 bytes in"""
    torch = _torch()
    rows, want, image = _wave_case(nch, kind)
    data = image[len(image) - nch * WAVE_N:]
    rspec, fspec = _wave_specs(layout, len(data), rows.dtype.itemsize)
    d_data = _put([data], fspec, np.uint8)
    d_rows = _put((nch, WAVE_N), rspec, rows.dtype)
    _ok(_L().vga_wave_deinterleave_pcm8_device(d_data.ptr, WAVE_N, nch, d_rows.ptr, kind, d_rows.pitch, _stream()))
    torch.cuda.synchronize()
    _eq(d_rows.rows(), want, "rows")
    d_rows.kept("rows", padding=True)
    d_data.unchanged("data")


# ====================================================================== BRWAV / BCWAV / BFWAV / prefetch banks
def _bank():
    """one small mixed bank: every kind and codec, rows under and over 16 bytes"""
    import nwwav_ref as ref
    from test_gpu_nwwav import make_bank
    from vgaudio_amd.nwwav import NwWaveBank
    files = [f for kind in range(5) for codec in range(3) for f in make_bank(900 + 3 * kind + codec, 1, kind=kind, codec=codec)]
    files += make_bank(990, 6, [5, 13, 27, 300, 1000, 2049])
    bank = NwWaveBank([img for img, _ in files])
    structs = [ref.read_image(img) for img, _ in files]
    assert {s["kind"] for s in structs} == set(range(5)) and {s["codec"] for s in structs} == {0, 1, 2}
    return bank, structs


def _bank_outputs(bank):
    """the three packed outputs in junk-filled allocations, by NwCodec: PCM8, PCM16, GC-ADPCM"""
    sizes = (int(bank.pcm8_bytes), int(bank.pcm16_samples) * 2, int(bank.adpcm_bytes))
    assert all(sizes)
    return sizes, [place((1, s), s, 0, np.uint8) for s in sizes]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["aligned", "files:base1"])
def test_nwwav_bank_read(layout):
    """vga_nwwav_bank_read_device: d_files, the one pointer of the call without a rule, at an odd base; every byte of
    each output inside [0, *_bytes) is a row's or zero, every byte outside unchanged"""
    from test_gpu_nwwav import host_order
    import nwwav_ref as ref
    torch = _torch()
    bank, structs = _bank()
    try:
        source = np.zeros(int(bank.file_offsets[len(bank.images) - 1]) + len(bank.images[-1]), np.uint8)
        assert _L().vga_nwwav_bank_source_bytes(bank._h) <= len(source)
        for f, img in enumerate(bank.images):
            at = int(bank.file_offsets[f])
            source[at:at + len(img)] = np.frombuffer(img, np.uint8)
        d_files = place([source], len(source), 1 if layout == "files:base1" else 0, np.uint8)
        sizes, outs = _bank_outputs(bank)
        want = [np.zeros(s, np.uint8) for s in sizes]
        r = 0
        for s in structs:
            for c in range(s["nch"]):
                row = host_order(s, c)
                at = int(bank.offsets[r]) * (2 if s["codec"] == ref.PCM16 else 1)
                want[s["codec"]][at:at + len(row)] = row
                r += 1
        _ok(_L().vga_nwwav_bank_read_device(bank._h, d_files.ptr, outs[2].ptr, outs[1].ptr, outs[0].ptr, _stream()))
        torch.cuda.synchronize()
        for codec, what in enumerate(("pcm8", "pcm16", "adpcm")):
            _eq(outs[codec].rows()[0], want[codec], what)
            outs[codec].kept(what, padding=True)
        d_files.unchanged("files")
    finally:
        bank.close()


# ====================================================================== refusals: one layout just outside each contract
@pytest.mark.gpu
def test_refuses_writer_file_pitch_at_8_mod_16():
    """three images 8 mod 16 apart: the NW stream (GC-ADPCM and PCM), HPS and IDSP writers name the pitch and write nothing"""
    L = _L()
    rcs, errs, outs = [], [], []

    def files(size):
        outs.append(place((3, size), _round_up(size, 16) + 8, 0, np.uint8))
        return outs[-1]

    adpcm, coefs, gain, sc, lc, seek, want, ne = _nw_case(2, 2, 3, 126)
    d_in, d_seek, tabs = place(adpcm, _round_up(adpcm.shape[1], 16), 0, np.uint8), place(seek, _round_up(2 * ne, 8), 0, np.int16), \
        _small_tables((coefs, gain, sc, lc), False)
    d = files(want.shape[1])
    rcs.append(L.vga_nwstm_write_device(C.byref(_nw_params(2, 126)), 2, 3, None, d_in.ptr, d_in.pitch, adpcm.shape[1], tabs[0].ptr,
                                        tabs[1].ptr, tabs[2].ptr, tabs[3].ptr, d_seek.ptr, d_seek.pitch, ne, d.ptr, d.pitch, _stream()))
    errs.append(_err())
    adpcm, pcm, coefs, gain, sc, want = _hps_case(8, 3, False)
    d_in, tabs = place(adpcm, _round_up(adpcm.shape[1], 16), 0, np.uint8), _small_tables((coefs, gain, sc), False)
    d = files(want.shape[1])
    rcs.append(L.vga_hps_write_device(C.byref(_hps_params(8, False)), 8, 3, d_in.ptr, d_in.pitch, adpcm.shape[1], tabs[0].ptr, tabs[1].ptr,
                                      tabs[2].ptr, None, 0, 0, d.ptr, d.pitch, _stream()))
    errs.append(_err())
    adpcm, coefs, gain, sc, lc, want = _idsp_case(3, 3, 0x10, 1)
    d_in, tabs = place(adpcm, _round_up(adpcm.shape[1], 16), 0, np.uint8), _small_tables((coefs, gain, sc, lc), False)
    d = files(want.shape[1])
    rcs.append(L.vga_idsp_write_device(C.byref(_idsp_params(0x10, 1)), 3, 3, d_in.ptr, d_in.pitch, adpcm.shape[1], tabs[0].ptr, tabs[1].ptr,
                                       tabs[2].ptr, tabs[3].ptr, d.ptr, d.pitch, _stream()))
    errs.append(_err())
    rows, _, want = _pcm_case(0, 256)
    d_in = place(rows, _round_up(PCM_N, 16), 0, rows.dtype)
    d = files(want.shape[1])
    rcs.append(L.vga_nwstm_pcm_write_device(C.byref(_pcm_params(0, 256)), PCM_KINDS[0][0], PCM_NCH, PCM_NF, None, d_in.ptr, PCM_KINDS[0][1],
                                            d_in.pitch, d.ptr, d.pitch, _stream()))
    errs.append(_err())
    _refused(rcs, errs, "file pitch", outs)


@pytest.mark.gpu
def test_refuses_a_pitch_below_the_row():
    """one writer and one reader: rows one byte closer than they are long"""
    from vgaudio_amd.nwstm import parse
    L = _L()
    adpcm, coefs, gain, sc, lc, seek, images, ne = _nw_case(1, 2, 3, 126)
    nb, size = adpcm.shape[1], images.shape[1]
    d_in, d_seek, tabs = place(adpcm, _round_up(nb, 16), 0, np.uint8), place(seek, _round_up(2 * ne, 8), 0, np.int16), \
        _small_tables((coefs, gain, sc, lc), False)
    d_out = place((3, size), _round_up(size, 16), 0, np.uint8)
    rcs = [L.vga_nwstm_write_device(C.byref(_nw_params(1, 126)), 2, 3, None, d_in.ptr, nb - 1, nb, tabs[0].ptr, tabs[1].ptr, tabs[2].ptr,
                                    tabs[3].ptr, d_seek.ptr, d_seek.pitch, ne, d_out.ptr, d_out.pitch, _stream())]
    errs = [_err()]
    info = parse(images[0].tobytes())
    d_files, d_rows = place(list(images), _round_up(size, 16), 0, np.uint8), place((6, nb), _round_up(nb, 16), 0, np.uint8)
    rcs.append(L.vga_nwstm_read_device(C.byref(info), d_files.ptr, d_files.pitch, 3, d_rows.ptr, nb - 1, _stream()))
    errs.append(_err())
    _refused(rcs, errs, "pitch <", [d_out, d_rows, d_in, d_files])


@pytest.mark.gpu
def test_refuses_a_bank_output_at_8_mod_16():
    """each of the bank's three outputs in turn 8 bytes past a 16-byte boundary"""
    bank, _ = _bank()
    try:
        source = np.zeros(max(int(_L().vga_nwwav_bank_source_bytes(bank._h)), 16), np.uint8)
        d_files = place([source], len(source), 0, np.uint8)
        sizes, outs = _bank_outputs(bank)
        rcs, errs = [], []
        for moved in range(3):
            ptr = [o.ptr + (8 if k == moved else 0) for k, o in enumerate(outs)]
            rcs.append(_L().vga_nwwav_bank_read_device(bank._h, d_files.ptr, ptr[2], ptr[1], ptr[0], _stream()))
            errs.append(_err())
        _refused(rcs, errs, "16-byte aligned", outs)
    finally:
        bank.close()


# ====================================================================== the CPU check: every granule is reached
ALL = {16, 8, 4, 2, 1}
# call (and kernel family, where one call has two) -> (the granules its geometry allows, why, [granule of every case])
GRANULE_CALLS = {
    "vga_nwstm_write_device": (ALL, "256-byte interleaves reach 16, 72-byte ones cap at 8",
                               lambda: [_nw_write_granule(t, *c) for t in NW_TARGETS for c in NW_WRITE_CASES]),
    "vga_nwstm_read_device": (ALL, "as the writer",
                              lambda: [_nw_read_granule(t, *c) for t in NW_TARGETS for c in NW_READ_CASES]),
    "vga_idsp_write_device": (ALL, "16-byte blocks reach 16; 56-byte blocks and the untrimmed whole channel (2408 bytes) cap at 8",
                              lambda: [_idsp_write_granule(*c[:3], t, c[3]) for t in (0, 1) for c in IDSP_WRITE_CASES]),
    "vga_idsp_read_device": (ALL, "as the writer",
                             lambda: [_idsp_read_granule(*c[:3], t, c[3]) for t in (0, 1) for c in IDSP_READ_CASES]),
    "vga_hps_write_device": (ALL, "headers, block headers and padded channel sizes are multiples of 0x20: no cap",
                             lambda: [_hps_write_granule(*c) for c in HPS_WRITE_CASES]),
    "vga_hps_read_device": (ALL, "as the writer", lambda: [_hps_read_granule(*c) for c in HPS_READ_CASES]),
    "vga_adx_write_device, one channel": (ALL, "a plain copy in one block; the audio starts 40 (version 4) or 36 bytes into the image",
                                          lambda: [_adx_write_granule(*c) for c in ADX_WRITE_CASES if c[1] == 1]),
    "vga_adx_write_device, several channels": ({2, 1}, "18- and 34-byte frames are the interleave: 2 at most",
                                               lambda: [_adx_write_granule(*c) for c in ADX_WRITE_CASES if c[1] > 1]),
}
for _k, (_codec, _kind, _big) in enumerate(PCM_KINDS):
    _name = f"PCM{16 if _codec == PCM16 else 8} {'big' if _big else 'little'}-endian, {'int16' if _kind == S16 else 'byte'} rows"
    GRANULE_CALLS[f"vga_nwstm_pcm_write_device, {_name}"] = (
        ALL, "256-sample interleaves reach 16; 255 and 258 samples cap at 1, 2 or 4",
        lambda k=_k: [_pcm_write_granule(*c) for c in PCM_WRITE_CASES if c[0] == k])
    GRANULE_CALLS[f"vga_nwstm_pcm_read_device, {_name}"] = (
        ALL, "as the writer", lambda k=_k: [_pcm_read_granule(*c) for c in PCM_READ_CASES if c[0] == k])


@pytest.mark.parametrize("call", sorted(GRANULE_CALLS))
def test_every_granule_is_reached(call):
    """from the base offsets, pitches, interleaves, last blocks and audio offsets the cases pass -- nothing else -- the
    granule the host must pick for each; a case that lands on the control's kernel proves nothing"""
    allowed, why, granules = GRANULE_CALLS[call]
    assert why
    got = set(granules())
    assert got == allowed, (call, sorted(allowed - got), sorted(got - allowed))


def test_the_aligned_layouts_take_the_widest_granule():
    """the control of every family is the 16-byte kernel wherever the geometry allows one"""
    assert _nw_write_granule(0, 2, 3, 448, "aligned") == 16 and _nw_write_granule(0, 2, 3, 126, "aligned") == 8
    assert _nw_read_granule(2, 3, 3, 448, "aligned") == 16 and _nw_read_granule(2, 3, 3, 126, "aligned") == 8
    assert _idsp_write_granule(3, 3, 0x10, 1, "aligned") == 16 and _idsp_write_granule(3, 3, 0x38, 1, "aligned") == 8
    assert _hps_write_granule(2, 3, False, "aligned") == 16 and _hps_read_granule(2, 3, False, "aligned") == 16
    assert _adx_write_granule(4, 1, 18, 0, "file:base8") == 16 and _adx_write_granule(4, 2, 18, 0, "aligned") == 2
    assert _pcm_write_granule(0, 256, "aligned") == 16 and _pcm_write_granule(2, 255, "aligned") == 1
    # with two 72-byte interleaves the padded last block is 16 bytes: only the interleave keeps these at 8
    assert _nw_geometry(2, 2, -126)[2]["audio_data_size"] - 2 * 72 == 16
    assert _nw_write_granule(2, 2, 3, -126, "aligned") == 8 and _nw_read_granule(2, 2, 3, -126, "aligned") == 8


def test_the_last_block_never_narrows_a_writers_granule():
    """interleave_images also ORs the last output block into its word.  Every writer pads the region to a multiple of 0x20
    (the NW streams) or of the interleave (IDSP), so whatever divides the interleave divides the last block: with the term
    dropped from the word no case here can fail, and none did on a scratch build.  Dropping the interleave is what
    test_nwstm_write[2-3--126-aligned] catches."""
    import nwstm_pcm_ref as pref
    shapes = [(G["interleave_size"], G["audio_data_size"]) for t in NW_TARGETS for spi in (448, 126, -126)
              for G in [_nw_geometry(t, 2, spi)[2]]]
    shapes += [(G["interleave"], G["audio_data_size"]) for b in IDSP_BLOCKS for trim in (0, 1) for G in [_idsp_geometry(3, b, trim)[1]]]
    shapes += [(G["interleave_size"], G["audio_data_size"]) for k in range(len(PCM_KINDS)) for spi in PCM_SPI for G in [_pcm_geometry(k, spi)]]
    assert len(shapes) == 27 and pref.PCM16 == PCM16
    for il, out in shapes:
        assert _granule(il, _last(out, il)) == _granule(il), (il, out)

"""Sets of GC-ADPCM files on the device (include/vgaudio_hip/gc_files.h): vga_gcadpcm_build_channels_device_v,
vga_dsp_write_device_v and vga_dsp_read_device_v on the packed rows of one set of twelve files (tests/gc_files_cases.py: the
smallest shapes at which each branch can go wrong).  Every channel's PCM, seek table and loop context must be the oracle's
gc_build_channel; every image the oracle's dsp_write and what vga_dsp_write_device writes for that file alone; what is read
back the oracle's dsp_read, and its decode the oracle's PCM.  All buffers are larger than needed and full of junk, and every
byte outside the rows, tables and images is compared afterwards.  The header is outside the lists the older test files
enumerate, so this file carries its own table (CASES); tests/test_gc_files_host.py holds that table to the header."""
import ctypes as C

import numpy as np
import pytest

import gc_files_cases as gf
from oracle import pyoracle as po
from test_gpu_device_streams import delay  # noqa: F401  (the calibrated GPU delay that makes a caller's stream busy)
from vgaudio_amd import _lib
from vgaudio_amd import dsp as vdsp
from vgaudio_amd.dsp import DspFileSet

pytestmark = pytest.mark.gpu

# function of the header -> the tests below that call it
CASES = {
    "vga_gc_files_layout_for": ["test_object_numbers_are_the_host_layouts"],
    "vga_gc_files_create": ["test_chain_matches_oracle", "test_object_numbers_are_the_host_layouts", "test_encode_files_returns_the_dsp_files"],
    "vga_gc_files_create_from_dsp": ["test_chain_matches_oracle", "test_reader_at_bases_8_mod_16", "test_reader_of_mixed_interleaves"],
    "vga_gc_files_destroy": ["test_chain_matches_oracle"],
    "vga_gc_files_totals_of": ["test_object_numbers_are_the_host_layouts"],
    "vga_gc_files_offsets": ["test_object_numbers_are_the_host_layouts"],
    "vga_gc_files_ragged": ["test_object_numbers_are_the_host_layouts", "test_chain_matches_oracle"],
    "vga_gcadpcm_build_channels_device_v": ["test_chain_matches_oracle", "test_bytes_do_not_depend_on_poison", "test_chain_on_a_busy_stream",
                                            "test_decode_is_skipped_when_nothing_needs_it", "test_refused_buffers_launch_nothing"],
    "vga_dsp_write_device_v": ["test_chain_matches_oracle", "test_bytes_do_not_depend_on_poison", "test_chain_on_a_busy_stream",
                               "test_null_arguments_mean_the_per_file_defaults", "test_refused_buffers_launch_nothing"],
    "vga_dsp_read_device_v": ["test_chain_matches_oracle", "test_bytes_do_not_depend_on_poison", "test_chain_on_a_busy_stream",
                              "test_reader_at_bases_8_mod_16", "test_reader_of_mixed_interleaves", "test_refused_buffers_launch_nothing"],
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


ALL_CONFIGS = [(name, trim) for name in sorted(gf.CONFIGS) for trim in (1, 0)]


def the_config(name, trim):
    return gf.config(*gf.CONFIGS[name], trim)


# ---------------------------------------------------------------- the oracle's side, computed once
_ref = {}


def reference():
    """per file: channels' coefficients, ADPCM, and gc_build_channel's PCM, seek table and loop context; gain and start context"""
    if not _ref:
        files = []
        pcm = po.synth_generate(260, 128, first_channel=40)
        c = 0
        for k, (nch, n, looping, ls, le, spacing) in enumerate(gf.FILES):
            p = po.gc_channel_params(n, bool(looping), ls, le, 0, spacing)
            chans = []
            for i in range(nch):
                x = pcm[(c + i) % 260, :n]
                coefs = po.gc_calculate_coefficients(x)
                adpcm = po.gc_encode(x, coefs)
                rc, lay, _, dec, seek, ctx = po.gc_build_channel(adpcm, coefs, p)
                assert rc == 0 and not lay.alignment_needed and len(dec) == n
                chans.append({"coefs": coefs, "adpcm": adpcm, "pcm": dec.copy(), "seek": seek.copy(), "ctx": ctx.copy(),
                              "gain": np.int16(100 * k + i - 300), "start": np.array([adpcm[0] if len(adpcm) else 0, 7 * i - 3, -k], np.int16)})
            files.append(chans)
            c += nch
        _ref["files"] = files
    return _ref["files"]


def flat(key, width=None):
    """one array over all channels of all files"""
    rows = [np.atleast_1d(ch[key]) for f in reference() for ch in f]
    return np.concatenate(rows).astype(np.int16) if width is None else np.stack(rows).astype(np.int16).reshape(-1)


_images = {}


def oracle_images(name, trim):
    """dsp_write's image of every file under the configuration (rc 0 for all twelve)"""
    if (name, trim) not in _images:
        spi, align = gf.CONFIGS[name]
        out = []
        for (nch, n, looping, ls, le, _), chans in zip(gf.FILES, reference()):
            p = po.dsp_params(gf.RATE, n, bool(looping), ls, le, spi, align, bool(trim))
            rc, img = po.dsp_write([ch["adpcm"] for ch in chans], np.stack([ch["coefs"] for ch in chans]), p,
                                   gain=np.array([ch["gain"] for ch in chans], np.int16), start_context=np.stack([ch["start"] for ch in chans]),
                                   loop_context=np.stack([ch["ctx"] if looping else np.zeros(3, np.int16) for ch in chans]))
            assert rc == 0, (name, trim, nch, n)
            out.append(img)
        _images[(name, trim)] = out
    return _images[(name, trim)]


def own_image(k, name, trim):
    """vga_dsp_write_device on file k alone"""
    t = torch()
    nch, n, looping, ls, le, _ = gf.FILES[k]
    chans = reference()[k]
    spi, align = gf.CONFIGS[name]
    p = _lib.DspParamsC(gf.RATE, n, looping, ls, le, spi, align, trim)
    lay = _lib.DspLayoutC()
    _lib.check(L().vga_dsp_layout_for(C.byref(p), nch, C.byref(lay)))
    nbytes = gf.byte_count(n)
    pitch = max(gf.up(nbytes, 16), 16)
    rows = np.zeros((nch, pitch), np.uint8)
    for i, ch in enumerate(chans):
        rows[i, :nbytes] = ch["adpcm"]
    d_rows, d_file = dev(rows), t.full((lay.file_size + 16,), JUNK, dtype=t.uint8, device="cuda")
    d_coefs, d_gain = dev(np.stack([ch["coefs"] for ch in chans])), dev(np.array([ch["gain"] for ch in chans], np.int16))
    d_start, d_loop = dev(np.stack([ch["start"] for ch in chans])), dev(np.stack([ch["ctx"] for ch in chans]))
    _lib.check(L().vga_dsp_write_device(d_rows.data_ptr(), pitch, nbytes, d_coefs.data_ptr(), d_gain.data_ptr(), d_start.data_ptr(),
                                        d_loop.data_ptr(), nch, C.byref(p), d_file.data_ptr(), None))
    t.cuda.synchronize()
    return host(d_file)[:lay.file_size]


# ---------------------------------------------------------------- one set and its junk-filled buffers
class Set:
    def __init__(self, name, trim):
        self.name, self.trim = name, trim
        self.files = [gf.gc_file(*f) for f in gf.FILES]
        self.s = DspFileSet(self.files, the_config(name, trim))
        self.m = gf.model(self.files, the_config(name, trim))
        self.t = self.s.totals
        self.chans = [ch for f in reference() for ch in f]
        nch = self.s.channels
        po_, ao_ = np.zeros(nch, np.int64), np.zeros(nch, np.int64)
        i64p = C.POINTER(C.c_int64)
        _lib.check(L().vga_gcadpcm_ragged_offsets(self.s.ragged, po_.ctypes.data_as(i64p), ao_.ctypes.data_as(i64p)))
        self.po, self.ao = po_, ao_

    def close(self):
        torch().cuda.synchronize()
        self.s.close()

    def adpcm_image(self):
        img = junk(self.t.adpcm_bytes)
        for ch, at in zip(self.chans, self.ao):
            img[at:at + ch["adpcm"].size] = ch["adpcm"]
        return img

    def check_rows(self, got, offsets, key, fill, what):
        own = np.zeros(got.size, bool)
        for c, (ch, at) in enumerate(zip(self.chans, offsets)):
            want = ch[key]
            own[at:at + want.size] = True
            assert np.array_equal(got[at:at + want.size], want), (what, key, "channel", c)
        assert np.all(got[~own] == fill), (what, key, "wrote outside the channels' own rows")

    def check_images(self, got, what, want=None):
        want = oracle_images(self.name, self.trim) if want is None else want
        own = np.zeros(got.size, bool)
        for f, (img, at) in enumerate(zip(want, self.s.image_offsets)):
            own[at:at + img.size] = True
            assert img.size == self.s.image_sizes[f]
            assert np.array_equal(got[at:at + img.size], img), (what, "file", f, gf.FILES[f])
        assert np.all(got[~own] == JUNK), (what, "wrote outside the images: a gap, the guard or the tail")

    def build_buffers(self, with_pcm=True):
        t = torch()
        nch = self.s.channels
        return {"adpcm": dev(self.adpcm_image()), "coefs": dev(flat("coefs", 16)),
                "pcm": dev(junk(self.t.pcm_samples, SENTINEL, np.int16)) if with_pcm else None,
                "seek": dev(junk(self.t.seek_shorts, SENTINEL, np.int16)), "ctx": dev(junk(nch * 3, SENTINEL, np.int16)),
                "status": t.zeros(2, dtype=t.int32, device="cuda"), "ws": dev(junk(self.t.build_workspace_bytes, 0xCD))}

    def run_build(self, b, stream=None):
        self.s.build_channels(b["adpcm"], b["coefs"], pcm=b["pcm"], seek=b["seek"], loop_context=b["ctx"], status=b["status"],
                              workspace=b["ws"], stream=stream)
        return b

    def build(self, with_pcm=True):
        return self.run_build(self.build_buffers(with_pcm))

    def check_build(self, b, what):
        nch = self.s.channels
        assert np.array_equal(host(b["adpcm"]), self.adpcm_image()), "d_adpcm is an input"
        self.check_rows(host(b["seek"]), self.s.seek_offsets, "seek", SENTINEL, what)
        ctx = host(b["ctx"])
        assert np.array_equal(ctx[:nch * 3], flat("ctx", 3)) and np.all(ctx[nch * 3:] == SENTINEL), what
        assert np.all(host(b["status"]) == 0)
        ws = host(b["ws"])
        if b["pcm"] is not None:
            self.check_rows(host(b["pcm"]), self.po, "pcm", SENTINEL, what)
            assert np.all(ws == 0xCD), (what, "the workspace is not needed when the caller takes the PCM")
        else:
            assert np.all(ws[self.t.build_workspace_bytes:] == 0xCD), (what, "wrote behind the workspace")
            pcm = ws[:self.t.build_workspace_bytes].view(np.int16)
            for c, (ch, at) in enumerate(zip(self.chans, self.po)):
                assert np.array_equal(pcm[at:at + ch["pcm"].size], ch["pcm"]), (what, "workspace PCM", c)

    def write_buffers(self):
        return {"adpcm": dev(self.adpcm_image()), "coefs": dev(flat("coefs", 16)), "gain": dev(flat("gain")), "start": dev(flat("start", 3)),
                "images": dev(junk(self.t.image_bytes))}

    def run_write(self, w, ctx, stream=None, defaults=False):
        if defaults:
            self.s.write_images(w["adpcm"], w["coefs"], w["images"], stream=stream)
        else:
            self.s.write_images(w["adpcm"], w["coefs"], w["images"], gain=w["gain"], start_context=w["start"], loop_context=ctx, stream=stream)
        return w["images"]

    def write(self, ctx, defaults=False):
        return self.run_write(self.write_buffers(), ctx, defaults=defaults)


class ReadSet:
    """a set made from the parsed headers of `images` (one array per file), its packed image buffer and junk-filled outputs"""

    def __init__(self, images, offsets=None):
        self.images = images
        self.infos = [vdsp.parse(img.tobytes()) for img in images]
        self.s = DspFileSet.from_infos(self.infos, offsets)
        self.t = self.s.totals
        self.want = []                                                 # per channel: dsp_read's row, coefficients, gain, contexts
        for img in images:
            rc, h, coefs, gain, sc, lc, rows = po.dsp_read(img.tobytes())
            assert rc == 0
            for i in range(h.channel_count):
                self.want.append({"adpcm": rows[i], "coefs": coefs[i], "gain": gain[i], "start": sc[i], "loop": lc[i], "samples": h.sample_count})
        nch = self.s.channels
        assert nch == len(self.want)
        po_, ao_ = np.zeros(max(nch, 1), np.int64), np.zeros(max(nch, 1), np.int64)
        i64p = C.POINTER(C.c_int64)
        _lib.check(L().vga_gcadpcm_ragged_offsets(self.s.ragged, po_.ctypes.data_as(i64p), ao_.ctypes.data_as(i64p)))
        self.po, self.ao = po_[:nch], ao_[:nch]

    def close(self):
        torch().cuda.synchronize()
        self.s.close()

    def packed(self):
        buf = junk(self.t.image_bytes, 0x5A)
        for img, at in zip(self.images, self.s.image_offsets):
            buf[at:at + img.size] = img
        return buf

    def read_buffers(self, d_images=None):
        t = torch()
        nch = self.s.channels
        return {"images": dev(self.packed()) if d_images is None else d_images, "adpcm": dev(junk(self.t.adpcm_bytes)),
                "coefs": dev(junk(nch * 16, SENTINEL, np.int16)), "gain": dev(junk(nch, SENTINEL, np.int16)),
                "start": dev(junk(nch * 3, SENTINEL, np.int16)), "loop": dev(junk(nch * 3, SENTINEL, np.int16)),
                "pcm": dev(junk(self.t.pcm_samples, SENTINEL, np.int16)), "status": t.zeros(1, dtype=t.int32, device="cuda")}

    def run_read(self, b, stream=None):
        """vga_dsp_read_device_v, then vga_gcadpcm_decode_device_v on what it delivered: no host round trip"""
        t = torch()
        self.s.read_images(b["images"], b["adpcm"], coefs=b["coefs"], gain=b["gain"], start_context=b["start"], loop_context=b["loop"],
                           stream=stream)
        st = C.c_void_p((stream if stream is not None else t.cuda.current_stream()).cuda_stream)
        _lib.check(L().vga_gcadpcm_decode_device_v(self.s.ragged, b["adpcm"].data_ptr(), b["coefs"].data_ptr(), None, None, b["pcm"].data_ptr(),
                                                   b["status"].data_ptr(), st))
        return b

    def read(self, d_images=None):
        return self.run_read(self.read_buffers(d_images))

    def check(self, b, what, images_in=None):
        nch = self.s.channels
        if images_in is not None:
            assert np.array_equal(host(b["images"]), images_in), "d_images is an input"
        got, own = host(b["adpcm"]), np.zeros(self.t.adpcm_bytes + EXTRA, bool)
        for c, (w, at) in enumerate(zip(self.want, self.ao)):
            own[at:at + w["adpcm"].size] = True
            assert np.array_equal(got[at:at + w["adpcm"].size], w["adpcm"]), (what, "row", c)
        assert np.all(got[~own] == JUNK), (what, "wrote outside the rows")
        for key, width in (("coefs", 16), ("gain", 1), ("start", 3), ("loop", 3)):
            v = host(b[key])
            want = np.concatenate([np.atleast_1d(w[key]) for w in self.want]).astype(np.int16)
            assert np.array_equal(v[:nch * width], want) and np.all(v[nch * width:] == SENTINEL), (what, key)
        pcm, own = host(b["pcm"]), np.zeros(self.t.pcm_samples + EXTRA, bool)
        assert int(host(b["status"])[0]) == 0
        for c, (w, at) in enumerate(zip(self.want, self.po)):
            n = w["samples"]
            own[at:at + n] = True
            assert np.array_equal(pcm[at:at + n], po.gc_decode(w["adpcm"], w["coefs"], n)), (what, "decoded row", c)
        assert np.all(pcm[~own] == SENTINEL), (what, "the decode wrote outside the rows")


def run_chain(name, trim, what, own=False):
    a = Set(name, trim)
    try:
        b = a.build(with_pcm=True)
        b2 = a.build(with_pcm=False)
        images = a.write(b["ctx"])
        torch().cuda.synchronize()
        a.check_build(b, (what, "build"))
        a.check_build(b2, (what, "build into the workspace"))
        got = host(images)
        a.check_images(got, (what, "write"))
        if own:
            a.check_images(got, (what, "the per-file call"), want=[own_image(k, name, trim) for k in range(len(gf.FILES))])
    finally:
        a.close()
    r = ReadSet([np.frombuffer(f, np.uint8) for f in a.s.split_images(got)])
    try:
        assert list(r.s.image_offsets) == list(a.s.image_offsets) and r.t.image_bytes == a.t.image_bytes
        rb = r.read(d_images=images)                                   # the writer's own buffer, on the device
        torch().cuda.synchronize()
        r.check(rb, (what, "read"), images_in=got)
    finally:
        r.close()


# ---------------------------------------------------------------- the chain against the oracle and the per-file calls
@pytest.mark.parametrize("name,trim", ALL_CONFIGS)
def test_chain_matches_oracle(name, trim):
    """build -> write -> (parse) -> read -> decode under every configuration"""
    imgs = oracle_images(name, trim)
    assert imgs[0].size == 98 and any(i.size % 16 for i in imgs)
    if name == "align4":                                               # header numbers only: same sizes unless the count grows past the data
        plain = oracle_images("oneblock", trim)
        assert any(not np.array_equal(x[:0x20], y[:0x20]) for x, y in zip(imgs, plain))
    run_chain(name, trim, (name, trim), own=True)


def test_object_numbers_are_the_host_layouts():
    for name, trim in (("blocks8", 1), ("align4", 0)):
        cfg = the_config(name, trim)
        a = Set(name, trim)
        try:
            fc, so, io, tot = DspFileSet.layout(a.files, cfg)
            assert all(getattr(tot, f) == getattr(a.t, f) for f, _ in tot._fields_)
            assert np.array_equal(fc, a.s.first_channel) and np.array_equal(so, a.s.seek_offsets) and np.array_equal(io, a.s.image_offsets)
            fc2, so2, io2 = np.zeros(tot.files, np.int32), np.zeros(tot.channels, np.int64), np.zeros(tot.files, np.int64)
            i64p = C.POINTER(C.c_int64)
            _lib.check(L().vga_gc_files_offsets(a.s._h, fc2.ctypes.data_as(C.POINTER(C.c_int)), so2.ctypes.data_as(i64p), io2.ctypes.data_as(i64p)))
            assert np.array_equal(fc2, fc) and np.array_equal(so2, so) and np.array_equal(io2, io)
            t2 = _lib.GcFilesTotalsC()
            _lib.check(L().vga_gc_files_totals_of(a.s._h, C.byref(t2)))
            assert all(getattr(t2, f) == getattr(tot, f) for f, _ in tot._fields_)
            # the borrowed ragged batch is the one vga_gcadpcm_ragged_create makes of the files' counts, repeated per channel
            r = L().vga_gc_files_ragged(a.s._h)
            assert r and L().vga_gcadpcm_ragged_channels(r) == tot.channels
            assert L().vga_gcadpcm_ragged_pcm_samples(r) == tot.pcm_samples and L().vga_gcadpcm_ragged_adpcm_bytes(r) == tot.adpcm_bytes
            assert list(a.po) == a.m["pcm_off"] and list(a.ao) == a.m["adpcm_off"]
        finally:
            a.close()


def test_reader_at_bases_8_mod_16():
    imgs = oracle_images("blocks16", 0)
    offsets, at = [], 8
    for img in imgs:
        offsets.append(at)
        at = gf.up(at + img.size, 16) + 8
    r = ReadSet(imgs, offsets)
    try:
        assert list(r.s.image_offsets) == offsets and all(o % 16 == 8 for o in offsets)
        b = r.read()
        torch().cuda.synchronize()
        r.check(b, "bases 8 mod 16", images_in=r.packed())
    finally:
        r.close()


def test_reader_of_mixed_interleaves():
    """files of one set with 1, 2 and 0x400 frames per interleave"""
    pools = [oracle_images("blocks8", 1), oracle_images("blocks16", 1), oracle_images("oneblock", 0)]
    imgs = [pools[k % 3][k] for k in range(len(gf.FILES))]
    r = ReadSet(imgs)
    try:
        assert len({i.frames_per_interleave for i in r.infos if i.channel_count > 1}) == 3
        b = r.read()
        torch().cuda.synchronize()
        r.check(b, "mixed interleaves", images_in=r.packed())
    finally:
        r.close()


def test_null_arguments_mean_the_per_file_defaults():
    """d_gain NULL: 0; d_start_context NULL: (the row's first byte, 0, 0); d_loop_context NULL: zeros"""
    a = Set("blocks8", 1)
    try:
        got = host(a.write(None, defaults=True))
        spi, align = gf.CONFIGS["blocks8"]
        want = []
        for (nch, n, looping, ls, le, _), chans in zip(gf.FILES, reference()):
            p = po.dsp_params(gf.RATE, n, bool(looping), ls, le, spi, align, True)
            start = np.array([[ch["adpcm"][0] if ch["adpcm"].size else 0, 0, 0] for ch in chans], np.int16)
            rc, img = po.dsp_write([ch["adpcm"] for ch in chans], np.stack([ch["coefs"] for ch in chans]), p, start_context=start)
            assert rc == 0
            want.append(img)
        a.check_images(got, "defaults", want=want)
    finally:
        a.close()


def test_decode_is_skipped_when_nothing_needs_it():
    """no seek table wanted, no loop start non-zero: the loop contexts are zeros and neither the workspace nor d_status is touched"""
    t = torch()
    files = [gf.gc_file(2, 100, 1, 0, 57, 14), gf.gc_file(1, 30, 0, 0, 0, 0)]
    s = DspFileSet(files, None)
    try:
        adpcm = dev(junk(s.totals.adpcm_bytes))
        coefs, ctx = dev(np.zeros(48, np.int16)), dev(junk(9, SENTINEL, np.int16))
        s.build_channels(adpcm, coefs, loop_context=ctx)               # no workspace at all
        t.cuda.synchronize()
        assert np.all(host(ctx)[:9] == 0) and np.all(host(ctx)[9:] == SENTINEL)
        seek = dev(junk(s.totals.seek_shorts, SENTINEL, np.int16))
        with pytest.raises(_lib.ArgumentError, match="workspace"):
            s.build_channels(adpcm, coefs, seek=seek)                  # a seek table needs the PCM
        with pytest.raises(_lib.InvalidOperationError):
            s.write_images(adpcm, coefs, dev(junk(64)))                # made without a configuration
        t.cuda.synchronize()
        assert np.all(host(seek) == SENTINEL)
    finally:
        s.close()


# ---------------------------------------------------------------- the Python mirror of Batch.cs in one call
def test_encode_files_returns_the_dsp_files():
    """gcadpcm.encode_files(dsp=...) -- upload, coefficients, encode, build, write on the device, one download -- gives what the
    per-file route DspWriter.GetFile(GcAdpcmFormat().EncodeFromPcm16(file)) gives"""
    from vgaudio_amd import gcadpcm
    pcm = po.synth_generate(8, 3000, first_channel=7)
    shapes = [(1, 3000, None), (2, 1400, (15, 1000)), (3, 29, (2, 20)), (2, 2999, (0, 2999)), (1, 57, (30, 40))]
    files, c = [], 0
    for nch, n, loop in shapes:
        f = gcadpcm.Pcm16Format([pcm[(c + i) % 8, :n] for i in range(nch)], 22050 + 1000 * nch)
        if loop:
            f.WithLoop(True, *loop)
        files.append(f)
        c += nch
    for cfg in (vdsp.DspConfiguration(), vdsp.DspConfiguration(SamplesPerInterleave=28, LoopPointAlignment=4, TrimFile=False)):
        got = gcadpcm.encode_files(files, dsp=cfg)
        want = [vdsp.DspWriter(cfg).GetFile(gcadpcm.GcAdpcmFormat().EncodeFromPcm16(f)) for f in files]
        assert [len(g) for g in got] == [len(w) for w in want]
        for k, (g, w) in enumerate(zip(got, want)):
            assert g == w, ("file", k, shapes[k])
    assert gcadpcm.encode_files([], dsp=vdsp.DspConfiguration()) == []


# ---------------------------------------------------------------- poison mode
def test_bytes_do_not_depend_on_poison():
    old = L().vga_testing_poison_allocations(0xA5)
    try:
        run_chain("blocks16", 1, "poison-a5")                          # (the sets are created under the mode: their tables are poisoned first)
    finally:
        torch().cuda.synchronize()
        L().vga_testing_poison_allocations(old if old >= 0 else -1)


# ---------------------------------------------------------------- a busy caller stream
def one_stream():
    """A stream for this file, taken so that the files that run after it find torch's stream pool as they would without it
    (tests/test_gpu_adx_ragged_device.py: two_streams): one whole turn of the pool with the imported `delay` fixture's, every
    stream used once, in order."""
    t = torch()
    taken = [t.cuda.Stream() for _ in range(POOL_STREAMS - 1)]
    for s in taken:
        with t.cuda.stream(s):
            t.zeros(1, device="cuda")
    t.cuda.synchronize()
    return taken[0]


def test_chain_on_a_busy_stream(delay):  # noqa: F811
    """build -> write -> read -> decode queued behind a delay on the caller's stream: no call waits for it"""
    t = torch()
    cycles, ms = delay
    a = Set("blocks8", 0)
    r = ReadSet(oracle_images("blocks8", 0))
    try:
        S = one_stream()
        with t.cuda.stream(S):
            for busy in (False, True):                                 # (warm first: every kernel has run once)
                b, w = a.build_buffers(with_pcm=False), a.write_buffers()
                rb = r.read_buffers(d_images=w["images"])
                S.synchronize()
                if busy:
                    t.cuda._sleep(cycles)
                a.run_build(b, stream=S)
                images = a.run_write(w, b["ctx"], stream=S)
                r.run_read(rb, stream=S)
                if busy:
                    assert not S.query(), "the caller's stream was idle when the calls returned (they waited for it)"
        S.synchronize()
        a.check_build(b, "busy stream")
        a.check_images(host(images), "busy stream")
        r.check(rb, "busy stream")
    finally:
        a.close()
        r.close()


# ---------------------------------------------------------------- refused buffers
def test_refused_buffers_launch_nothing():
    t = torch()
    ARG = _lib.VGA_ERR_ARGUMENT
    a = Set("blocks8", 1)
    r = ReadSet(oracle_images("blocks8", 1))
    try:
        h, need = a.s._h, a.t.build_workspace_bytes
        adpcm, coefs = dev(a.adpcm_image()), dev(flat("coefs", 16))
        pcm, seek = dev(junk(a.t.pcm_samples, SENTINEL, np.int16)), dev(junk(a.t.seek_shorts, SENTINEL, np.int16))
        ctx, ws, images = dev(junk(a.s.channels * 3, SENTINEL, np.int16)), dev(junk(need, 0xCD)), dev(junk(a.t.image_bytes))
        A, K, P, S, X, W, I = (v.data_ptr() for v in (adpcm, coefs, pcm, seek, ctx, ws, images))
        build, write, read = L().vga_gcadpcm_build_channels_device_v, L().vga_dsp_write_device_v, L().vga_dsp_read_device_v
        assert build(h, A + 8, K, P, S, X, None, W, need, None) == ARG
        assert build(h, A, K, P + 8, S, X, None, W, need, None) == ARG
        assert build(h, A, K, P, S + 8, X, None, W, need, None) == ARG
        assert build(h, A, K, None, S, X, None, W + 8, need, None) == ARG
        assert build(h, A, K, None, S, X, None, W, need - 16, None) == ARG
        assert build(h, A, K, None, S, X, None, None, need, None) == ARG
        assert build(h, None, K, P, S, X, None, W, need, None) == ARG and build(h, A, None, P, S, X, None, W, need, None) == ARG
        assert write(h, A + 8, K, None, None, None, I, None) == ARG and write(h, A, K, None, None, None, I + 8, None) == ARG
        assert write(h, None, K, None, None, None, I, None) == ARG and write(h, A, None, None, None, None, I, None) == ARG
        assert write(h, A, K, None, None, None, None, None) == ARG
        assert read(h, I, A, None, None, None, None, None) == _lib.VGA_ERR_INVALID_OP      # not a set made from headers
        rows, packed = dev(junk(r.t.adpcm_bytes)), dev(r.packed())
        assert read(r.s._h, packed.data_ptr() + 8, rows.data_ptr(), None, None, None, None, None) == ARG
        assert read(r.s._h, packed.data_ptr(), rows.data_ptr() + 8, None, None, None, None, None) == ARG
        assert read(r.s._h, None, rows.data_ptr(), None, None, None, None, None) == ARG
        assert read(r.s._h, packed.data_ptr(), None, None, None, None, None, None) == ARG
        assert write(r.s._h, A, K, None, None, None, I, None) == _lib.VGA_ERR_INVALID_OP
        t.cuda.synchronize()
        assert np.all(host(pcm) == SENTINEL) and np.all(host(seek) == SENTINEL) and np.all(host(ctx) == SENTINEL)
        assert np.all(host(ws) == 0xCD) and np.all(host(images) == JUNK) and np.all(host(rows) == JUNK)
        # exactly at the minimum: buffers of the totals' sizes
        ws_min, img_min = dev(junk(need, 0xCD)[:need]), dev(junk(a.t.image_bytes)[:a.t.image_bytes])
        adpcm_min = dev(a.adpcm_image()[:a.t.adpcm_bytes])
        assert build(h, adpcm_min.data_ptr(), K, None, S, X, None, ws_min.data_ptr(), need, None) == 0
        assert write(h, adpcm_min.data_ptr(), K, dev(flat("gain")).data_ptr(), dev(flat("start", 3)).data_ptr(), X, img_min.data_ptr(), None) == 0
        t.cuda.synchronize()
        a.check_images(np.concatenate([host(img_min), np.full(EXTRA, JUNK, np.uint8)]), "at the minimum")
    finally:
        a.close()
        r.close()

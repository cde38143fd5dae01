"""Sets of IDSP files on the device (include/vgaudio_hip_files/idsp_files.h): vga_idsp_write_device_v and vga_idsp_read_device_v on
the packed rows of one set of files (tests/idsp_files_cases.py: the smallest shapes at which each branch can go wrong, block
sizes 0, 8, 0x10 and 0x4000, trim on and off).  Every image must be tests/gc_containers_ref.idsp_image's (the restatement of
IdspWriter) and what vga_idsp_write_device writes for that file alone; every row read back must be vga_idsp_read_device's
and gc_containers_ref.idsp_parse's.  All buffers are larger than needed and full of junk, and every byte outside the images,
rows and per-channel arrays is compared afterwards.  The header is outside the lists the older test files enumerate, so this
file carries its own table (CASES); tests/test_idsp_files_host.py holds that table to the header."""
import ctypes as C

import numpy as np
import pytest

import gc_aligned_cases as ga
import gc_containers_ref as gr
import idsp_files_cases as ic
from oracle import pyoracle as po
from test_gpu_device_streams import delay  # noqa: F401  (the calibrated GPU delay that makes a caller's stream busy)
from vgaudio_amd import _lib
from vgaudio_amd.gcadpcm import AlignedFileSet
from vgaudio_amd.idsp import IdspFileSet

pytestmark = pytest.mark.gpu

# function of the header -> the tests below that call it
CASES = {
    "vga_idsp_files_layout_for": ["test_object_numbers_are_the_host_layouts"],
    "vga_idsp_files_create": ["test_images_are_the_reference_writers_and_the_per_file_calls", "test_object_numbers_are_the_host_layouts"],
    "vga_idsp_files_create_from_infos": ["test_read_gives_the_per_file_rows_and_the_decode_follows", "test_refused_calls_launch_nothing"],
    "vga_idsp_files_destroy": ["test_images_are_the_reference_writers_and_the_per_file_calls"],
    "vga_idsp_files_totals_of": ["test_object_numbers_are_the_host_layouts"],
    "vga_idsp_files_offsets": ["test_object_numbers_are_the_host_layouts"],
    "vga_idsp_files_gc_files": ["test_object_numbers_are_the_host_layouts", "test_chain_from_pcm_stays_on_the_device"],
    "vga_idsp_files_ragged": ["test_object_numbers_are_the_host_layouts", "test_read_gives_the_per_file_rows_and_the_decode_follows"],
    "vga_idsp_write_device_v": [
        "test_images_are_the_reference_writers_and_the_per_file_calls", "test_chain_from_pcm_stays_on_the_device",
        "test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream", "test_two_calls_on_two_streams",
        "test_refused_calls_launch_nothing", "test_an_empty_set_launches_nothing", "test_write_files_and_read_files_are_the_mirrors"],
    "vga_idsp_read_device_v": [
        "test_read_gives_the_per_file_rows_and_the_decode_follows", "test_foreign_geometry_is_read_not_refused",
        "test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream", "test_refused_calls_launch_nothing",
        "test_an_empty_set_launches_nothing", "test_write_files_and_read_files_are_the_mirrors"],
    "vga_idsp_files_write_regions_for": ["test_object_numbers_are_the_host_layouts"],
    "vga_idsp_files_read_regions_for": ["test_foreign_geometry_is_read_not_refused"],
    "vga_idsp_files_stats": ["test_images_are_the_reference_writers_and_the_per_file_calls", "test_read_gives_the_per_file_rows_and_the_decode_follows",
                             "test_an_empty_set_launches_nothing", "test_refused_calls_launch_nothing"],
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
    return torch().from_numpy(np.array(a)).cuda()                      # (a copy: the shared inputs are read only)


def host(t):
    return t.cpu().numpy()


def stream_ptr(stream=None):
    return C.c_void_p((stream if stream is not None else torch().cuda.current_stream()).cuda_stream)


def ptr(t):
    return t.data_ptr() if t is not None else None


def row_offsets(ragged, nch):
    """(pcm offsets, adpcm offsets) of a ragged batch's rows"""
    po_, ao = np.zeros(max(nch, 1), np.int64), np.zeros(max(nch, 1), np.int64)
    i64p = C.POINTER(C.c_int64)
    _lib.check(L().vga_gcadpcm_ragged_offsets(ragged, po_.ctypes.data_as(i64p), ao.ctypes.data_as(i64p)))
    return po_[:nch], ao[:nch]


# ---------------------------------------------------------------- one set for writing
_per_file = {}


class WriteSet:
    def __init__(self, name):
        self.name = name
        self.i = ic.inputs(name)                                       # shared, read only
        self.cfg, self.files, self.m = self.i["cfg"], self.i["files"], self.i["model"]
        self.s = IdspFileSet(self.files, configuration=self.cfg)
        self.t = self.s.totals
        self.nch = len(self.m["counts"])

    def close(self):
        self.s.close()

    def inputs(self):
        """the packed rows (junk in every gap and guard) and the per-channel arrays, on the device"""
        adpcm = np.full(self.t.adpcm_bytes + EXTRA, JUNK, np.uint8)
        for c, row in enumerate(self.i["rows"]):
            adpcm[self.m["adpcm_off"][c]:self.m["adpcm_off"][c] + len(row)] = row
        return {"adpcm": dev(adpcm), "coefs": dev(self.i["coefs"]), "gain": dev(self.i["gain"]), "start": dev(self.i["start"]),
                "loop": dev(self.i["loop"])}

    def images(self, fill=JUNK):
        return torch().full((self.t.image_bytes + EXTRA,), fill, dtype=torch().uint8, device="cuda")

    def run(self, b, images, nulls=False, stream=None):
        _lib.check(L().vga_idsp_write_device_v(self.s._h, ptr(b["adpcm"]), ptr(b["coefs"]), None if nulls else ptr(b["gain"]),
                                               None if nulls else ptr(b["start"]), None if nulls else ptr(b["loop"]), ptr(images),
                                               stream_ptr(stream)))
        return images

    def per_file(self, nulls):
        """vga_idsp_write_device on every file alone, from the same rows: one `bytes` per file.  (That call refuses a NULL start
        context for rows of no bytes, where the set writes zeros: such a file gets an explicit (0, 0, 0).)"""
        key = (self.name, nulls)
        if key in _per_file:
            return _per_file[key]
        t, out, c = torch(), [], 0
        for f, lay in zip(self.files, self.m["layouts"]):
            nch, p = f.channels, ic.params_of(f, self.cfg)
            n = gr.bytes_of(lay["channel_sample_count"])
            pitch = max(ic.up(n, 16), 16)
            rows = np.full((nch, pitch), 0x5A, np.uint8)
            for i in range(nch):
                rows[i, :n] = self.i["rows"][c + i]
            d_rows, d_coefs = dev(rows), dev(self.i["coefs"][c:c + nch])
            d_gain, d_start, d_loop = dev(self.i["gain"][c:c + nch]), dev(self.i["start"][c:c + nch]), dev(self.i["loop"][c:c + nch])
            zeros = dev(np.zeros((nch, 3), np.int16))
            image = t.full((lay["file_size"] + 16,), JUNK, dtype=t.uint8, device="cuda")
            _lib.check(L().vga_idsp_write_device(C.byref(p), nch, 1, ptr(d_rows) if n else None, pitch, n, ptr(d_coefs),
                                                 None if nulls else ptr(d_gain), (None if n else ptr(zeros)) if nulls else ptr(d_start),
                                                 None if nulls else ptr(d_loop), ptr(image), lay["file_size"], stream_ptr()))
            t.cuda.synchronize()
            got = host(image)
            assert np.all(got[lay["file_size"]:] == JUNK)
            out.append(got[:lay["file_size"]].tobytes())
            c += nch
        _per_file[key] = out
        return out

    def check(self, images, nulls, what, fill=JUNK):
        """every image is the per-file call's and the reference writer's; every byte outside the images is untouched"""
        got = host(images)
        mask = np.ones(got.size, bool)
        want_own, want_ref = self.per_file(nulls), self.i["nulls" if nulls else "given"]
        for f, (at, size) in enumerate(zip(self.m["image_off"], self.m["image_size"])):
            image = got[at:at + size].tobytes()
            assert image == want_ref[f], (what, "file", f, "differs from the reference writer")
            assert image == want_own[f], (what, "file", f, "differs from vga_idsp_write_device")
            mask[at:at + size] = False
        assert np.all(got[mask] == fill), (what, "bytes outside the images were written")


# ---------------------------------------------------------------- 1. write, per configuration
@pytest.mark.parametrize("name", sorted(ic.CONFIGS))
def test_images_are_the_reference_writers_and_the_per_file_calls(name):
    a = WriteSet(name)
    try:
        b = a.inputs()
        given = a.run(b, a.images())
        assert a.s.stats()[3] == 2                                     # two launches whatever the number of files
        nulls = a.run(b, a.images(), nulls=True)
        torch().cuda.synchronize()
        a.check(given, False, (name, "arrays given"))
        a.check(nulls, True, (name, "NULL arrays"))
        assert host(given)[:4].tobytes() == b"IDSP"
        items, wide, table_bytes, _ = a.s.stats()
        assert items >= len(a.files) - 1 and table_bytes > 0 and (wide > 0) == (a.cfg.block_size % 16 == 0)
        assert np.array_equal(host(b["adpcm"]), host(a.inputs()["adpcm"]))     # the inputs are read only
    finally:
        a.close()


# ---------------------------------------------------------------- 2. the chain
def pcm_files(shapes):
    from vgaudio_amd import gcadpcm
    pcm = ga.source_pcm()
    files, c = [], 0
    for nch, n, loop in shapes:
        f = gcadpcm.Pcm16Format([pcm[(c + i) % 64, :n] for i in range(nch)], 22050 + 1000 * nch)
        if loop:
            f.WithLoop(True, *loop)
        files.append(f)
        c += nch
    return files


SHAPES = [(2, 1400, (15, 1000)), (1, 3000, None), (4, 29, (2, 20)), (2, 500, (28, 400)), (1, 5, None)]


@pytest.mark.parametrize("block,trim", [(0x10, True), (8, False), (0, True)])
def test_chain_from_pcm_stays_on_the_device(block, trim):
    """vga_gcadpcm_coefs_device_v -> vga_gcadpcm_encode_device_v -> vga_gcadpcm_align_channels_device_v -> vga_idsp_write_device_v on
    one set, no host step between them: the images are the host mirror's IdspWriter.GetFile on the same files"""
    from vgaudio_amd import gcadpcm, idsp
    t = torch()
    files = pcm_files(SHAPES)
    s = IdspFileSet([(f.ChannelCount, f.SampleRate, f.SampleCount, f.Looping, f.LoopStart if f.Looping else 0, f.LoopEnd if f.Looping else 0)
                     for f in files], ic.config(block, int(trim)))
    al = AlignedFileSet(s.gc_files())
    try:
        tot, nch = al.totals, al.channels
        assert (tot.out_adpcm_bytes, nch) == (s.totals.adpcm_bytes, s.channels)
        assert list(al.offsets("out")[1]) == list(row_offsets(s.ragged, nch)[1])
        pin, ain = al.offsets("in")
        pcm, c = np.zeros(tot.pcm_samples, np.int16), 0
        for f in files:
            for ch in f.Channels:
                pcm[pin[c]:pin[c] + f.SampleCount] = np.asarray(ch, np.int16)[:f.SampleCount]
                c += 1
        new = lambda n, dtype, fill: t.full((max(int(n), 16) + EXTRA,), fill, dtype=dtype, device="cuda")
        d_pcm, coefs, adpcm = dev(pcm), new(nch * 16, t.int16, SENTINEL), new(tot.adpcm_bytes, t.uint8, JUNK)
        out, ctx = new(tot.out_adpcm_bytes, t.uint8, JUNK), new(nch * 3, t.int16, SENTINEL)
        ws = t.empty(max(L().vga_gcadpcm_ragged_coefs_workspace_bytes(al.ragged_in), tot.workspace_bytes, 16), dtype=t.uint8, device="cuda")
        images, st = new(s.totals.image_bytes, t.uint8, JUNK), stream_ptr()
        _lib.check(L().vga_gcadpcm_coefs_device_v(al.ragged_in, ptr(d_pcm), ptr(coefs), ptr(ws), ws.numel(), st))
        _lib.check(L().vga_gcadpcm_encode_device_v(al.ragged_in, ptr(d_pcm), ptr(coefs), None, None, ptr(adpcm), st))
        al.align_channels(adpcm, coefs, out, loop_context=ctx, workspace=ws)
        # the start context is the unaligned stream's first byte: gathered on the device, no host step
        start = t.zeros(nch * 3, dtype=t.int16, device="cuda")
        start.view(-1, 3)[:, 0] = adpcm[dev(np.ascontiguousarray(ain, dtype=np.int64))].to(t.int16)
        _lib.check(L().vga_idsp_write_device_v(s._h, ptr(out), ptr(coefs), None, ptr(start), ptr(ctx), ptr(images), st))
        t.cuda.synchronize()
        got, mask = host(images), np.ones(images.numel(), bool)
        writer = idsp.IdspWriter(idsp.IdspConfiguration(BlockSize=block, TrimFile=trim))
        for k, (f, at, size) in enumerate(zip(files, s.image_offsets, s.image_sizes)):
            want = writer.GetFile(gcadpcm.GcAdpcmFormat().EncodeFromPcm16(f))
            assert got[at:at + size].tobytes() == want, (block, trim, "file", k)
            mask[at:at + size] = False
        assert np.all(got[mask] == JUNK)
    finally:
        al.close()
        s.close()


# ---------------------------------------------------------------- 3. read
def packed_images(files, offsets, total, fill=0x3C):
    packed = np.full(total, fill, np.uint8)
    for f, o in zip(files, offsets):
        packed[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return packed


def check_read(r, files, infos, what, want_rows=None):
    """a read of `files` through the set r: the rows are the per-file call's and gc_containers_ref.idsp_parse's, nothing else is
    written, the per-channel arrays are the infos', and the decode follows on the device"""
    t = torch()
    nch, tot = r.channels, r.totals
    packed = packed_images(files, r.image_offsets, tot.image_bytes + EXTRA)
    d_images = dev(packed)
    rows = t.full((tot.adpcm_bytes + EXTRA,), JUNK, dtype=t.uint8, device="cuda")
    coefs, gain = t.full((nch * 16 + EXTRA,), SENTINEL, dtype=t.int16, device="cuda"), t.full((nch + EXTRA,), SENTINEL, dtype=t.int16, device="cuda")
    start, loop = (t.full((nch * 3 + EXTRA,), SENTINEL, dtype=t.int16, device="cuda") for _ in range(2))
    r.read(d_images, rows, coefs, gain, start, loop)
    assert r.stats()[3] == 2
    rows2 = t.full((tot.adpcm_bytes + EXTRA,), JUNK, dtype=t.uint8, device="cuda")
    r.read(d_images, rows2)                                            # the per-channel arrays are optional
    assert r.stats()[3] == 1
    t.cuda.synchronize()
    got, mask, c = host(rows), np.ones(tot.adpcm_bytes + EXTRA, bool), 0
    po_, ao = row_offsets(r.ragged, nch)
    want_coefs, want_gain, want_start, want_loop, audio = [], [], [], [], []
    for f, info in zip(files, infos):
        k, n = info.channel_count, info.adpcm_bytes
        pitch = max(ic.up(n, 16), 16)
        own = t.full((k, pitch), JUNK, dtype=t.uint8, device="cuda")
        d_file = dev(np.frombuffer(f, np.uint8))
        _lib.check(L().vga_idsp_read_device(C.byref(info), ptr(d_file), len(f), 1, ptr(own), pitch, stream_ptr()))
        t.cuda.synchronize()
        own, ref = host(own), gr.idsp_parse(bytes(f))["audio"]
        for i in range(k):
            assert got[ao[c + i]:ao[c + i] + n].tobytes() == ref[i], (what, "channel", c + i, "differs from the reference reader")
            assert np.array_equal(got[ao[c + i]:ao[c + i] + n], own[i, :n]), (what, "channel", c + i, "differs from vga_idsp_read_device")
            mask[ao[c + i]:ao[c + i] + n] = False
            audio.append(ref[i])
            want_coefs.append(list(info.coefs[i])), want_gain.append(info.gain[i])
            want_start.append(list(info.start_context[i])), want_loop.append(list(info.loop_context[i]))
        c += k
    assert np.all(got[mask] == JUNK), (what, "bytes outside the rows were written")
    assert np.array_equal(got, host(rows2))
    assert np.array_equal(host(coefs)[:nch * 16].reshape(nch, 16), np.array(want_coefs, np.int16)) and np.all(host(coefs)[nch * 16:] == SENTINEL)
    assert np.array_equal(host(gain)[:nch], np.array(want_gain, np.int16)) and np.all(host(gain)[nch:] == SENTINEL)
    assert np.array_equal(host(start)[:nch * 3].reshape(nch, 3), np.array(want_start, np.int16)) and np.all(host(start)[nch * 3:] == SENTINEL)
    assert np.array_equal(host(loop)[:nch * 3].reshape(nch, 3), np.array(want_loop, np.int16)) and np.all(host(loop)[nch * 3:] == SENTINEL)
    assert np.all(host(d_images) == packed)                            # the images are read only
    # the decode follows without a host round trip
    pcm = t.full((tot.pcm_samples + EXTRA,), SENTINEL, dtype=t.int16, device="cuda")
    status = t.zeros(1, dtype=t.int32, device="cuda")
    _lib.check(L().vga_gcadpcm_decode_device_v(r.ragged, ptr(rows), ptr(coefs), None, None, ptr(pcm), ptr(status), stream_ptr()))
    t.cuda.synchronize()
    dec, c = host(pcm), 0
    for info in infos:
        for i in range(info.channel_count):
            n = info.sample_count
            if n:
                want = po.gc_decode(np.frombuffer(audio[c], np.uint8), np.array(want_coefs[c], np.int16), n)
                assert np.array_equal(dec[po_[c]:po_[c] + n], want), (what, "decode of channel", c)
            c += 1


@pytest.mark.parametrize("offsets", ["packed", "caller"])
@pytest.mark.parametrize("name", ["b0", "b8", "b16", "b4000"])
def test_read_gives_the_per_file_rows_and_the_decode_follows(name, offsets):
    i = ic.inputs(name)
    files = i["given"]
    infos = [ic.parse(f) for f in files]
    offs, at = None, 8
    if offsets == "caller":                                            # multiples of 8 that are not multiples of 16
        offs = []
        for f in files:
            offs.append(at)
            at = ic.up(at + len(f), 16) + 8
    r = IdspFileSet.from_infos(infos, offs)
    try:
        assert list(r.image_offsets) == (offs if offs is not None else i["model"]["image_off"])
        check_read(r, files, infos, (name, offsets))
        wide = r.stats()[1]
        assert (wide > 0) == (offsets == "packed" and name in ("b16", "b4000", "b0"))
    finally:
        r.close()


def test_foreign_geometry_is_read_not_refused():
    """interleaves, bytes per channel and audio offsets that are multiples of nothing, at image offsets at any byte: the general
    form of the read kernel; whatever vga_idsp_read_device reads, the set reads"""
    files = [ic.foreign_image(2, 12, 580, 1000)[0], ic.foreign_image(2, 7, 575, 1000)[0], ic.foreign_image(3, 0x10, 2288, 4000, pad=5)[0],
             ic.foreign_image(1, 0, 1001, 1750)[0], ic.foreign_image(2, 0x10, 32, 100)[0], ic.foreign_image(5, 0x10, 2304, 4000)[0],
             ic.foreign_image(1, 3, 5000, 8000)[0], ic.foreign_image(2, 8, 576, 1000)[0]]
    infos = [ic.parse(f) for f in files]
    for offs in (None, np.cumsum([3] + [len(f) + 5 for f in files[:-1]]).tolist()):
        r = IdspFileSet.from_infos(infos, offs)
        try:
            check_read(r, files, infos, ("foreign", offs is None))
            ptrs, n = (C.c_void_p * len(infos))(*[C.addressof(i) for i in infos]), C.c_int64()
            o = np.ascontiguousarray(offs, np.int64).ctypes.data_as(C.POINTER(C.c_int64)) if offs is not None else None
            _lib.check(L().vga_idsp_files_read_regions_for(ptrs, len(infos), o, None, 0, C.byref(n)))
            regions = (_lib.IdspFilesRegionC * n.value)()
            _lib.check(L().vga_idsp_files_read_regions_for(ptrs, len(infos), o, regions, n.value, C.byref(n)))
            assert n.value == r.stats()[0]
            assert {x.granule for x in regions} == {1, 8, 16} if offs is None else 1 in {x.granule for x in regions}
        finally:
            r.close()


# ---------------------------------------------------------------- 4. the object's numbers, the empty set
def test_object_numbers_are_the_host_layouts():
    for name in ("b8", "b4000"):
        a = WriteSet(name)
        try:
            fc, io, tot = IdspFileSet.layout(a.files, configuration=a.cfg)
            assert list(a.s.first_channel) == list(fc) and list(a.s.image_offsets) == list(io)
            assert all(getattr(a.t, k) == getattr(tot, k) for k, _ in tot._fields_)
            assert a.s.image_sizes == a.m["image_size"]
            rg = a.s.ragged
            assert rg and L().vga_gcadpcm_ragged_channels(rg) == a.nch and L().vga_gcadpcm_ragged_adpcm_bytes(rg) == tot.adpcm_bytes
            assert list(row_offsets(rg, a.nch)[1]) == a.m["adpcm_off"]
            for g, f in zip(a.s.gc_files(), a.files):
                assert (g.channels, g.sample_rate) == (f.channels, f.sample_rate) and bytes(g.channel) == bytes(ic.file_layout(f, a.cfg)[1].channel)
            arr, n = (_lib.IdspFileC * len(a.files))(*a.files), C.c_int64()
            _lib.check(L().vga_idsp_files_write_regions_for(arr, len(a.files), C.byref(a.cfg), None, 0, C.byref(n)))
            assert n.value == len(a.files) + a.s.stats()[0]            # the object's items are the host call's
        finally:
            a.close()


def test_an_empty_set_launches_nothing():
    t = torch()
    s, r = IdspFileSet([], configuration=ic.config(0x10)), IdspFileSet.from_infos([])
    try:
        images = t.full((512,), JUNK, dtype=t.uint8, device="cuda")
        assert L().vga_idsp_write_device_v(s._h, ptr(images), ptr(images), None, None, None, ptr(images), stream_ptr()) == 0
        assert s.stats()[3] == 0
        assert L().vga_idsp_read_device_v(r._h, ptr(images), ptr(images), None, None, None, None, stream_ptr()) == 0
        assert r.stats()[3] == 0
        assert L().vga_idsp_write_device_v(s._h, None, None, None, None, None, None, None) == 0
        t.cuda.synchronize()
        assert np.all(host(images) == JUNK)
        assert s.totals.image_bytes == 256 and s.gc_files() == []
    finally:
        s.close()
        r.close()


# ---------------------------------------------------------------- 5. poison mode
@pytest.mark.parametrize("value", [0xA5, 0xFF])
def test_bytes_do_not_depend_on_poison(value):
    old = L().vga_testing_poison_allocations(value)
    try:
        a = WriteSet("b16")                                            # (created under the mode: its tables are poisoned first)
        try:
            images = a.run(a.inputs(), a.images(value ^ 0x3C))
            torch().cuda.synchronize()
            a.check(images, False, ("poison", value), fill=value ^ 0x3C)
        finally:
            a.close()
        i = ic.inputs("b8")
        files = i["given"]
        infos = [ic.parse(f) for f in files]
        r = IdspFileSet.from_infos(infos)
        try:
            packed = packed_images(files, r.image_offsets, r.totals.image_bytes, value)
            rows = torch().full((r.totals.adpcm_bytes,), value ^ 0x3C, dtype=torch().uint8, device="cuda")
            r.read(dev(packed), rows)
            torch().cuda.synchronize()
            got, c = host(rows), 0
            ao = row_offsets(r.ragged, r.channels)[1]
            for f, info in zip(files, infos):
                for row in gr.idsp_parse(f)["audio"]:
                    assert got[ao[c]:ao[c] + info.adpcm_bytes].tobytes() == row
                    got[ao[c]:ao[c] + info.adpcm_bytes] = value ^ 0x3C
                    c += 1
            assert np.all(got == value ^ 0x3C)
        finally:
            r.close()
    finally:
        torch().cuda.synchronize()
        L().vga_testing_poison_allocations(old if old >= 0 else -1)


# ---------------------------------------------------------------- 6. streams
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


def test_calls_on_a_busy_stream(delay):  # noqa: F811
    """both calls queued behind a delay on the caller's stream: they do not wait for it, and they are ordered after it -- their
    inputs are written on the same stream after the delay"""
    t = torch()
    cycles, ms = delay
    a = WriteSet("b16")
    files = a.i["given"]
    infos = [ic.parse(f) for f in files]
    r = IdspFileSet.from_infos(infos)
    try:
        (S,) = some_streams(1)
        b = a.inputs()
        source, d_packed = b["adpcm"], dev(packed_images(files, r.image_offsets, r.totals.image_bytes))
        with t.cuda.stream(S):
            for busy in (False, True):                                 # (warm first: every kernel has run once)
                b["adpcm"] = t.zeros_like(source)
                d_images = t.zeros_like(d_packed)
                images, rows = a.images(), t.full((r.totals.adpcm_bytes,), JUNK, dtype=t.uint8, device="cuda")
                S.synchronize()
                if busy:
                    t.cuda._sleep(cycles)
                b["adpcm"].copy_(source, non_blocking=True)            # the inputs arrive behind the delay
                d_images.copy_(d_packed, non_blocking=True)
                a.run(b, images, stream=S)
                r.read(d_images, rows, stream=S)
                if busy:
                    assert not S.query(), "the caller's stream was idle when the calls returned (they waited for it)"
        S.synchronize()
        a.check(images, False, "busy stream")
        got, ao, c = host(rows), row_offsets(r.ragged, r.channels)[1], 0
        for f, info in zip(files, infos):
            for row in gr.idsp_parse(f)["audio"]:
                assert got[ao[c]:ao[c] + info.adpcm_bytes].tobytes() == row, ("busy stream: row", c)
                c += 1
    finally:
        r.close()
        a.close()


def test_two_calls_on_two_streams():
    """one object, two streams"""
    t = torch()
    a = WriteSet("b8")
    try:
        S1, S2 = some_streams(2)
        b, i1, i2 = a.inputs(), a.images(), a.images(0x11)
        t.cuda.synchronize()
        a.run(b, i1, stream=S1)
        a.run(b, i2, nulls=True, stream=S2)
        S1.synchronize()
        S2.synchronize()
        a.check(i1, False, "stream 1")
        a.check(i2, True, "stream 2", fill=0x11)
    finally:
        a.close()


# ---------------------------------------------------------------- 7. refused calls
def test_refused_calls_launch_nothing():
    t = torch()
    ARG, OP = _lib.VGA_ERR_ARGUMENT, -4
    a = WriteSet("b16")
    r = IdspFileSet.from_infos([ic.parse(f) for f in a.i["given"]])
    try:
        b, images = a.inputs(), a.images()
        rows = t.full((a.t.adpcm_bytes + EXTRA,), JUNK, dtype=t.uint8, device="cuda")
        A, K, I, R = ptr(b["adpcm"]), ptr(b["coefs"]), ptr(images), ptr(rows)
        write, read = L().vga_idsp_write_device_v, L().vga_idsp_read_device_v
        assert write(a.s._h, A + 8, K, None, None, None, I, None) == ARG
        assert write(a.s._h, A, K, None, None, None, I + 8, None) == ARG
        assert write(a.s._h, None, K, None, None, None, I, None) == ARG and write(a.s._h, A, None, None, None, None, I, None) == ARG
        assert write(a.s._h, A, K, None, None, None, None, None) == ARG
        assert write(r._h, A, K, None, None, None, I, None) == OP           # a set for reading
        assert read(a.s._h, I, R, None, None, None, None, None) == OP       # a set for writing
        assert read(r._h, I + 8, R, None, None, None, None, None) == ARG and read(r._h, I, R + 8, None, None, None, None, None) == ARG
        assert read(r._h, None, R, None, None, None, None, None) == ARG and read(r._h, I, None, None, None, None, None, None) == ARG
        assert a.s.stats()[3] == 0
        assert L().vga_idsp_files_gc_files(r._h, (_lib.GcFileC * r.files)()) == OP
        t.cuda.synchronize()
        assert np.all(host(images) == JUNK) and np.all(host(rows) == JUNK)
        # exactly at the minimum: buffers of the totals' sizes
        exact = b["adpcm"][:a.t.adpcm_bytes].clone()
        out = t.full((a.t.image_bytes,), JUNK, dtype=t.uint8, device="cuda")
        assert write(a.s._h, ptr(exact), K, ptr(b["gain"]), ptr(b["start"]), ptr(b["loop"]), ptr(out), None) == 0
        t.cuda.synchronize()
        a.check(out, False, "at the minimum")
    finally:
        r.close()
        a.close()


# ---------------------------------------------------------------- 8. the Python mirror
@pytest.mark.parametrize("block,trim", [(0x10, True), (8, False), (0, False)])
def test_write_files_and_read_files_are_the_mirrors(block, trim):
    """idsp.write_files -- upload, coefficients, encode, align and assemble on the device, one download -- gives per file what
    IdspWriter(configuration).GetFile(GcAdpcmFormat().EncodeFromPcm16(file)) returns, and idsp.read_files what IdspReader().ReadFormat
    returns, the PCM what its ToPcm16 gives"""
    from vgaudio_amd import gcadpcm, idsp
    files = pcm_files(SHAPES)
    cfg = lambda: idsp.IdspConfiguration(BlockSize=block, TrimFile=trim)
    got = idsp.write_files(files, cfg())
    writer = idsp.IdspWriter(cfg())
    for k, f in enumerate(files):
        assert got[k] == writer.GetFile(gcadpcm.GcAdpcmFormat().EncodeFromPcm16(f)), ("file", k)
    assert idsp.write_files([]) == [] and idsp.read_files([]) == []
    formats, pcm = idsp.read_files(got, pcm=True)
    for k, (image, fmt) in enumerate(zip(got, formats)):
        want = idsp.IdspReader().ReadFormat(image)
        assert (fmt.ChannelCount, fmt.SampleRate, fmt.SampleCount, fmt.Looping) == (want.ChannelCount, want.SampleRate, want.SampleCount, want.Looping)
        decoded = want.ToPcm16()
        for c in range(want.ChannelCount):
            assert np.array_equal(fmt.Channels[c].GetAdpcmAudio(), want.Channels[c].GetAdpcmAudio()), ("file", k, "channel", c)
            assert np.array_equal(fmt.Channels[c].Coefs, want.Channels[c].Coefs)
            assert np.array_equal(pcm[k][c], np.asarray(decoded.Channels[c], np.int16)[:want.SampleCount]), ("file", k, "pcm", c)

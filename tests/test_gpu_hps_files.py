"""Sets of HPS files on the device (include/vgaudio_hip_files/hps_files.h): vga_hps_write_device_v and vga_hps_read_device_v on
the packed rows of one set of files (tests/hps_files_cases.py: the smallest shapes at which the block map can go wrong).  Every
image must be tests/gc_containers_ref.hps_image's (the restatement of HpsWriter) and what vga_hps_write_device writes for that
file alone; every row read back must be vga_hps_read_device's and gc_containers_ref.hps_parse's.  All buffers are larger than
needed and full of junk, and every byte outside the images, rows and per-channel arrays is compared afterwards.  The header
is outside the lists the older test files enumerate, so this file carries its own table (CASES);
tests/test_hps_files_host.py holds that table to the header."""
import ctypes as C

import numpy as np
import pytest

import far_memory as fm
import gc_aligned_cases as ga
import gc_containers_ref as gr
import hps_files_cases as hc
from oracle import pyoracle as po
from test_gpu_device_streams import delay  # noqa: F401  (the calibrated GPU delay that makes a caller's stream busy)
from vgaudio_amd import _lib
from vgaudio_amd.gcadpcm import AlignedFileSet
from vgaudio_amd.hps import HpsFileSet

pytestmark = pytest.mark.gpu

# function of the header -> the tests below that call it
CASES = {
    "vga_hps_files_layout_for": ["test_object_numbers_are_the_host_layouts"],
    "vga_hps_files_create": ["test_images_are_the_reference_writers_and_the_per_file_calls", "test_object_numbers_are_the_host_layouts"],
    "vga_hps_files_create_from_infos": ["test_read_gives_the_per_file_rows_and_the_decode_follows", "test_refused_calls_launch_nothing"],
    "vga_hps_files_destroy": ["test_images_are_the_reference_writers_and_the_per_file_calls"],
    "vga_hps_files_totals_of": ["test_object_numbers_are_the_host_layouts"],
    "vga_hps_files_offsets": ["test_object_numbers_are_the_host_layouts"],
    "vga_hps_files_gc_files": ["test_object_numbers_are_the_host_layouts", "test_chain_from_pcm_stays_on_the_device"],
    "vga_hps_files_ragged": ["test_object_numbers_are_the_host_layouts", "test_read_gives_the_per_file_rows_and_the_decode_follows"],
    "vga_hps_write_device_v": [
        "test_images_are_the_reference_writers_and_the_per_file_calls", "test_chain_from_pcm_stays_on_the_device",
        "test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream", "test_two_calls_on_two_streams",
        "test_refused_calls_launch_nothing", "test_an_empty_set_launches_nothing", "test_write_files_and_read_files_are_the_mirrors"],
    "vga_hps_read_device_v": [
        "test_read_gives_the_per_file_rows_and_the_decode_follows", "test_foreign_geometry_is_read_not_refused",
        "test_read_at_offsets_around_4_gib", "test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream",
        "test_refused_calls_launch_nothing", "test_an_empty_set_launches_nothing", "test_write_files_and_read_files_are_the_mirrors"],
    "vga_hps_files_write_regions_for": ["test_object_numbers_are_the_host_layouts"],
    "vga_hps_files_read_regions_for": ["test_foreign_geometry_is_read_not_refused"],
    "vga_hps_files_stats": ["test_images_are_the_reference_writers_and_the_per_file_calls", "test_read_gives_the_per_file_rows_and_the_decode_follows",
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


# ---------------------------------------------------------------- the set for writing
_per_file = {}


class WriteSet:
    def __init__(self):
        self.i = hc.inputs()                                           # shared, read only
        self.files, self.m = self.i["files"], self.i["model"]
        self.s = HpsFileSet(self.files)
        self.t = self.s.totals
        self.nch = len(self.m["counts"])

    def close(self):
        self.s.close()

    def inputs(self):
        """the packed rows (junk in every gap and guard) and the per-channel arrays, on the device"""
        adpcm = np.full(self.t.adpcm_bytes + EXTRA, JUNK, np.uint8)
        pcm = np.full(self.t.pcm_samples + EXTRA, SENTINEL, np.int16)
        for c, (row, samples) in enumerate(zip(self.i["rows"], self.i["pcm"])):
            adpcm[self.m["adpcm_off"][c]:self.m["adpcm_off"][c] + len(row)] = row
            pcm[self.m["pcm_off"][c]:self.m["pcm_off"][c] + len(samples)] = samples
        return {"adpcm": dev(adpcm), "pcm": dev(pcm), "coefs": dev(self.i["coefs"]), "gain": dev(self.i["gain"]),
                "start": dev(self.i["start"])}

    def images(self, fill=JUNK):
        return torch().full((self.t.image_bytes + EXTRA,), fill, dtype=torch().uint8, device="cuda")

    def run(self, b, images, nulls=False, stream=None):
        _lib.check(L().vga_hps_write_device_v(self.s._h, ptr(b["adpcm"]), ptr(b["coefs"]), None if nulls else ptr(b["gain"]),
                                              None if nulls else ptr(b["start"]), None if nulls else ptr(b["pcm"]), ptr(images),
                                              stream_ptr(stream)))
        return images

    def per_file(self, nulls):
        """vga_hps_write_device on every file alone (the small shapes of the case table), from the same rows: one `bytes` per
        file"""
        if nulls in _per_file:
            return _per_file[nulls]
        t, out, c = torch(), [], 0
        for f, lay in zip(self.files, self.m["layouts"]):
            nch, p = f.channels, hc.params_of(f)
            count = lay["channel_sample_count"]
            n = gr.bytes_of(count)
            pitch, ppitch = hc.up(n, 16), hc.up(count, 8)
            rows, pcm = np.full((nch, pitch), 0x5A, np.uint8), np.full((nch, ppitch), SENTINEL, np.int16)
            for i in range(nch):
                rows[i, :n] = self.i["rows"][c + i]
                pcm[i, :count] = self.i["pcm"][c + i]
            d_rows, d_pcm, d_coefs = dev(rows), dev(pcm), dev(self.i["coefs"][c:c + nch])
            d_gain, d_start = dev(self.i["gain"][c:c + nch]), dev(self.i["start"][c:c + nch])
            image = t.full((lay["file_size"] + 16,), JUNK, dtype=t.uint8, device="cuda")
            _lib.check(L().vga_hps_write_device(C.byref(p), nch, 1, ptr(d_rows), pitch, n, ptr(d_coefs), None if nulls else ptr(d_gain),
                                                None if nulls else ptr(d_start), None if nulls else ptr(d_pcm), ppitch, count, ptr(image),
                                                lay["file_size"], stream_ptr()))
            t.cuda.synchronize()
            got = host(image)
            assert np.all(got[lay["file_size"]:] == JUNK)
            out.append(got[:lay["file_size"]].tobytes())
            c += nch
        _per_file[nulls] = out
        return out

    def check(self, images, nulls, what, fill=JUNK):
        """every image is the per-file call's and the reference writer's; every byte outside the images is untouched"""
        got = host(images)
        mask = np.ones(got.size, bool)
        want_own, want_ref = self.per_file(nulls), self.i["nulls" if nulls else "given"]
        for f, (at, size) in enumerate(zip(self.m["image_off"], self.m["image_size"])):
            image = got[at:at + size].tobytes()
            assert image == want_ref[f], (what, "file", hc.ORDER[f], "differs from the reference writer")
            assert image == want_own[f], (what, "file", hc.ORDER[f], "differs from vga_hps_write_device")
            mask[at:at + size] = False
        assert np.all(got[mask] == fill), (what, "bytes outside the images were written")


# ---------------------------------------------------------------- 1. write
def test_images_are_the_reference_writers_and_the_per_file_calls():
    a = WriteSet()
    try:
        b = a.inputs()
        given = a.run(b, a.images())
        assert a.s.stats()[3] == 2                                     # two launches whatever the number of files
        nulls = a.run(b, a.images(), nulls=True)
        assert a.s.stats()[3] == 2
        torch().cuda.synchronize()
        a.check(given, False, "arrays given")
        a.check(nulls, True, "NULL arrays")
        assert host(given)[:8].tobytes() == b" HALPST\0"
        items, blocks, table_bytes, _ = a.s.stats()
        assert blocks == a.m["blocks"] == a.t.blocks and items > blocks and table_bytes >= 32 * blocks
        fresh = a.inputs()
        assert np.array_equal(host(b["adpcm"]), host(fresh["adpcm"])) and np.array_equal(host(b["pcm"]), host(fresh["pcm"]))   # read only
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


# The block headers' hist1 / hist2 come from the aligned set's PCM output.  HpsWriter takes them from the Pcm field the format
# carried INTO the alignment, which holds the same samples up to the last frame the re-encode keeps (loop_end / 14 * 14) and
# nothing, or other samples, behind it: the file that needs the re-encode, (16, 20000, 14000 .. 20000), has its loop block, the
# last one, start at 14336, inside the kept part, so that both say the same.
SHAPES = [(2, 1400, (0, 1000)), (1, 3000, None), (16, 20000, (14000, 20000)), (8, 29000, (14336, 29000)), (4, 29, None), (1, 5, None)]


def test_chain_from_pcm_stays_on_the_device():
    """vga_gcadpcm_coefs_device_v -> vga_gcadpcm_encode_device_v -> vga_gcadpcm_align_channels_device_v -> vga_hps_write_device_v on
    one set, no host step between them: the images are the host mirror's HpsWriter.GetFile on the same files"""
    from vgaudio_amd import gcadpcm, hps
    t = torch()
    files = pcm_files(SHAPES)
    s = HpsFileSet([(f.ChannelCount, f.SampleRate, f.SampleCount, f.Looping, f.LoopStart if f.Looping else 0, f.LoopEnd if f.Looping else 0)
                    for f in files])
    al = AlignedFileSet(s.gc_files())
    try:
        tot, nch = al.totals, al.channels
        lays = [HpsFileSet.file_layout(hc.hps_file(f.ChannelCount, f.SampleCount, int(f.Looping), f.LoopStart if f.Looping else 0,
                                                   f.LoopEnd if f.Looping else 0)) for f in files]
        assert [bool(x.alignment_needed) for x in lays] == [False, False, True, False, False, False]
        assert lays[2].loop_block == 2 and lays[3].block_count == 3 and lays[3].loop_block == 1
        assert (tot.out_adpcm_bytes, tot.out_pcm_samples, nch) == (s.totals.adpcm_bytes, s.totals.pcm_samples, s.channels)
        assert list(al.offsets("out")[1]) == list(row_offsets(s.ragged, nch)[1])
        pin, ain = al.offsets("in")
        pcm, c = np.zeros(tot.pcm_samples, np.int16), 0
        for f in files:
            for ch in f.Channels:
                pcm[pin[c]:pin[c] + f.SampleCount] = np.asarray(ch, np.int16)[:f.SampleCount]
                c += 1
        new = lambda n, dtype, fill: t.full((max(int(n), 16) + EXTRA,), fill, dtype=dtype, device="cuda")
        d_pcm, coefs, adpcm = dev(pcm), new(nch * 16, t.int16, SENTINEL), new(tot.adpcm_bytes, t.uint8, JUNK)
        out, pcm_out = new(tot.out_adpcm_bytes, t.uint8, JUNK), new(tot.out_pcm_samples, t.int16, SENTINEL)
        ws = t.empty(max(L().vga_gcadpcm_ragged_coefs_workspace_bytes(al.ragged_in), tot.workspace_bytes, 16), dtype=t.uint8, device="cuda")
        images, st = new(s.totals.image_bytes, t.uint8, JUNK), stream_ptr()
        _lib.check(L().vga_gcadpcm_coefs_device_v(al.ragged_in, ptr(d_pcm), ptr(coefs), ptr(ws), ws.numel(), st))
        _lib.check(L().vga_gcadpcm_encode_device_v(al.ragged_in, ptr(d_pcm), ptr(coefs), None, None, ptr(adpcm), st))
        al.align_channels(adpcm, coefs, out, pcm=pcm_out, workspace=ws)
        # the start context is the unaligned stream's first byte: gathered on the device, no host step
        start = t.zeros(nch * 3, dtype=t.int16, device="cuda")
        start.view(-1, 3)[:, 0] = adpcm[dev(np.ascontiguousarray(ain, dtype=np.int64))].to(t.int16)
        _lib.check(L().vga_hps_write_device_v(s._h, ptr(out), ptr(coefs), None, ptr(start), ptr(pcm_out), ptr(images), st))
        t.cuda.synchronize()
        got, mask = host(images), np.ones(images.numel(), bool)
        writer = hps.HpsWriter()
        for k, (f, at, size) in enumerate(zip(files, s.image_offsets, s.image_sizes)):
            want = writer.GetFile(gcadpcm.GcAdpcmFormat().EncodeFromPcm16(f))
            assert got[at:at + size].tobytes() == want, ("file", k)
            mask[at:at + size] = False
        assert np.all(got[mask] == JUNK)
    finally:
        al.close()
        s.close()


# ---------------------------------------------------------------- 3. read
def packed_images(r, files, total, fill=0x3C):
    """the images where the set r expects them"""
    packed = np.full(total, fill, np.uint8)
    for f, o, n in zip(files, r.image_offsets, r.image_sizes):
        assert 0 < n <= len(f)
        packed[o:o + n] = np.frombuffer(f, np.uint8)[:n]
    return packed


_rows = {}


def per_file_rows(files, parsed):
    """vga_hps_read_device on every file alone: per file the rows (channels, adpcm_bytes); computed once per list of files"""
    key = tuple(id(f) for f in files)
    if key not in _rows:
        t, out = torch(), []
        for f, (info, blocks) in zip(files, parsed):
            k, n = info.channel_count, info.adpcm_bytes
            pitch = hc.up(n, 16)
            own = t.full((k, pitch), JUNK, dtype=t.uint8, device="cuda")
            d_file = dev(np.frombuffer(f, np.uint8))
            _lib.check(L().vga_hps_read_device(C.byref(info), blocks, ptr(d_file), len(f), 1, ptr(own), pitch, stream_ptr()))
            t.cuda.synchronize()
            out.append(host(own)[:, :n].copy())
        _rows[key] = (files, out)                                      # (the list is kept: its id stays its own)
    return _rows[key][1]


def check_rows(r, got, files, parsed, what, fill=JUNK):
    """the rows are the per-file call's and gc_containers_ref.hps_parse's, and nothing else was written"""
    mask, c = np.ones(got.size, bool), 0
    ao = row_offsets(r.ragged, r.channels)[1]
    own = per_file_rows(files, parsed)
    for k, (f, (info, _)) in enumerate(zip(files, parsed)):
        ref, n = gr.hps_parse(bytes(f))["audio"], info.adpcm_bytes
        for i in range(info.channel_count):
            assert got[ao[c]:ao[c] + n].tobytes() == ref[i], (what, "channel", c, "differs from the reference reader")
            assert np.array_equal(got[ao[c]:ao[c] + n], own[k][i]), (what, "channel", c, "differs from vga_hps_read_device")
            mask[ao[c]:ao[c] + n] = False
            c += 1
    assert np.all(got[mask] == fill), (what, "bytes outside the rows were written")


def check_read(r, files, parsed, what):
    """a read of `files` through the set r: the rows, the per-channel arrays (the infos'), and the decode that follows on the
    device"""
    t = torch()
    nch, tot = r.channels, r.totals
    packed = packed_images(r, files, tot.image_bytes + EXTRA)
    d_images = dev(packed)
    rows = t.full((tot.adpcm_bytes + EXTRA,), JUNK, dtype=t.uint8, device="cuda")
    coefs, gain = t.full((nch * 16 + EXTRA,), SENTINEL, dtype=t.int16, device="cuda"), t.full((nch + EXTRA,), SENTINEL, dtype=t.int16, device="cuda")
    start, loop = (t.full((nch * 3 + EXTRA,), SENTINEL, dtype=t.int16, device="cuda") for _ in range(2))
    r.read(d_images, rows, coefs, gain, start, loop)
    assert r.stats()[3] == 2                                           # at most two launches whatever the number of files
    rows2 = t.full((tot.adpcm_bytes + EXTRA,), JUNK, dtype=t.uint8, device="cuda")
    r.read(d_images, rows2)                                            # the per-channel arrays are optional
    assert r.stats()[3] == 1
    t.cuda.synchronize()
    got = host(rows)
    check_rows(r, got, files, parsed, what)
    assert np.array_equal(got, host(rows2))
    want = {k: [] for k in ("coefs", "gain", "start", "loop")}
    for info, _ in parsed:
        for i in range(info.channel_count):
            want["coefs"].append(list(info.coefs[i])), want["gain"].append(info.gain[i])
            want["start"].append(list(info.start_context[i])), want["loop"].append(list(info.loop_context[i]))
    for name, tensor, width in (("coefs", coefs, 16), ("gain", gain, 1), ("start", start, 3), ("loop", loop, 3)):
        h = host(tensor)
        assert np.array_equal(h[:nch * width], np.array(want[name], np.int16).reshape(-1)) and np.all(h[nch * width:] == SENTINEL), name
    assert np.all(host(d_images) == packed)                            # the images are read only
    # the decode follows without a host round trip
    pcm = t.full((tot.pcm_samples + EXTRA,), SENTINEL, dtype=t.int16, device="cuda")
    status = t.zeros(1, dtype=t.int32, device="cuda")
    _lib.check(L().vga_gcadpcm_decode_device_v(r.ragged, ptr(rows), ptr(coefs), None, None, ptr(pcm), ptr(status), stream_ptr()))
    t.cuda.synchronize()
    dec, c = host(pcm), 0
    po_, ao = row_offsets(r.ragged, nch)
    for info, _ in parsed:
        for i in range(info.channel_count):
            n = min(info.sample_count, 300)                            # (the head of every row: the decode is tested elsewhere)
            expect = po.gc_decode(got[ao[c]:ao[c] + gr.bytes_of(n)], np.array(want["coefs"][c], np.int16), n)
            assert np.array_equal(dec[po_[c]:po_[c] + n], expect), (what, "decode of channel", c)
            c += 1


def written():
    files = hc.inputs()["given"]
    if "parsed" not in _rows:
        _rows["parsed"] = [hc.parse(f) for f in files]
    return files, _rows["parsed"]


@pytest.mark.parametrize("offsets", ["packed", "caller"])
def test_read_gives_the_per_file_rows_and_the_decode_follows(offsets):
    files, parsed = written()
    offs, at = None, 16
    if offsets == "caller":                                            # multiples of 16 in another order of gaps, then any byte
        offs = []
        for k, f in enumerate(files):
            offs.append(at)
            at = hc.up(at + len(f), 16) + (48 if k % 2 else 5)
    r = HpsFileSet.from_infos(parsed, offs)
    try:
        assert list(r.image_offsets) == (offs if offs is not None else hc.inputs()["model"]["image_off"])
        assert r.image_sizes == [len(f) for f in files]
        assert r.totals.blocks == hc.inputs()["model"]["blocks"]
        check_read(r, files, parsed, offsets)
    finally:
        r.close()


def foreign():
    if "foreign" not in _rows:
        files = [hc.foreign_image(2, [0x40 * 5, 0x40 * 3 + 7])[0], hc.foreign_image(3, [0x45, 0x40 * 200, 30], stride_pad=4)[0],
                 hc.foreign_image(1, [0x40 * 40 + 4, 0x40], stride_pad=1)[0], hc.foreign_image(5, [0x40 * 300 + 20], stride_pad=16)[0]]
        _rows["foreign"] = (files, [hc.parse(f) for f in files])
    return _rows["foreign"]


def test_foreign_geometry_is_read_not_refused():
    """block sizes, channel strides and row offsets that are multiples of nothing, at image offsets at any byte: the general form
    of the gather; whatever vga_hps_read_device reads, the set reads"""
    files, parsed = foreign()
    for offs in (None, np.cumsum([3] + [len(f) + 5 for f in files[:-1]]).tolist()):
        r = HpsFileSet.from_infos(parsed, offs)
        try:
            check_read(r, files, parsed, ("foreign", offs is None))
            infos = (C.c_void_p * len(parsed))(*[C.addressof(i) for i, _ in parsed])
            tables = (C.c_void_p * len(parsed))(*[C.addressof(b) for _, b in parsed])
            n = C.c_int64()
            o = np.ascontiguousarray(offs, np.int64).ctypes.data_as(C.POINTER(C.c_int64)) if offs is not None else None
            _lib.check(L().vga_hps_files_read_regions_for(infos, tables, len(parsed), o, None, 0, C.byref(n)))
            regions = (_lib.HpsFilesRegionC * n.value)()
            _lib.check(L().vga_hps_files_read_regions_for(infos, tables, len(parsed), o, regions, n.value, C.byref(n)))
            assert n.value == r.stats()[0]
            assert {x.granule for x in regions} == ({1, 16} if offs is None else {1})
        finally:
            r.close()


def test_read_at_offsets_around_4_gib():
    """images at the caller's offsets on both sides of 2^32 of one allocation: an offset formed in 32 bits lands elsewhere in it"""
    t = torch()
    files, parsed = written()
    pick = [hc.ORDER.index(k) for k in ("later", "full+1", "wide", "mono", "short")]
    files, parsed = [files[k] for k in pick], [parsed[k] for k in pick]
    base = (1 << 32) - len(files[0]) // 2 // 16 * 16 - 5               # the first image straddles 2^32, at an odd byte
    offs, at = [], base
    for k, f in enumerate(files):
        offs.append(at)
        at = hc.up(at + len(f), 16) + (0 if k % 2 else 7)
    extent = at + (1 << 20)
    fm.need(extent)
    far = fm.FarBuffer(extent)
    r = HpsFileSet.from_infos(parsed, offs)
    try:
        assert r.totals.image_bytes <= extent and list(r.image_offsets) == offs
        windows = [far.put(o, np.frombuffer(f, np.uint8)) for o, f in zip(offs, files)]
        rows = t.full((r.totals.adpcm_bytes + EXTRA,), JUNK, dtype=t.uint8, device="cuda")
        _lib.check(L().vga_hps_read_device_v(r._h, far.ptr, ptr(rows), None, None, None, None, stream_ptr()))
        t.cuda.synchronize()
        got, c = host(rows), 0
        mask, ao = np.ones(got.size, bool), row_offsets(r.ragged, r.channels)[1]
        for f, (info, _) in zip(files, parsed):
            for row in gr.hps_parse(bytes(f))["audio"]:
                assert got[ao[c]:ao[c] + info.adpcm_bytes].tobytes() == row, ("far", "channel", c)
                mask[ao[c]:ao[c] + info.adpcm_bytes] = False
                c += 1
        assert np.all(got[mask] == JUNK)
        assert far.untouched(windows) is None                          # the images are read only
    finally:
        r.close()
        far.free()


# ---------------------------------------------------------------- 4. the object's numbers, the empty set
def test_object_numbers_are_the_host_layouts():
    a = WriteSet()
    try:
        fc, io, fb, tot = HpsFileSet.layout(a.files)
        assert list(a.s.first_channel) == list(fc) and list(a.s.image_offsets) == list(io) and list(a.s.first_block) == list(fb)
        assert all(getattr(a.t, k) == getattr(tot, k) for k, _ in tot._fields_)
        assert a.s.image_sizes == a.m["image_size"]
        rg = a.s.ragged
        assert rg and L().vga_gcadpcm_ragged_channels(rg) == a.nch and L().vga_gcadpcm_ragged_adpcm_bytes(rg) == tot.adpcm_bytes
        po_, ao = row_offsets(rg, a.nch)
        assert list(ao) == a.m["adpcm_off"] and list(po_) == a.m["pcm_off"]
        for g, f in zip(a.s.gc_files(), a.files):
            assert (g.channels, g.sample_rate) == (f.channels, f.sample_rate) and bytes(g.channel) == bytes(hc.file_layout(f)[1].channel)
        arr, n = (_lib.HpsFileC * len(a.files))(*a.files), C.c_int64()
        _lib.check(L().vga_hps_files_write_regions_for(arr, len(a.files), None, 0, C.byref(n)))
        items, blocks, _, _ = a.s.stats()
        assert n.value == len(a.files) + blocks + items                # the object's tables are the host call's
    finally:
        a.close()


def test_an_empty_set_launches_nothing():
    t = torch()
    s, r = HpsFileSet([]), HpsFileSet.from_infos([])
    try:
        images = t.full((512,), JUNK, dtype=t.uint8, device="cuda")
        assert L().vga_hps_write_device_v(s._h, ptr(images), ptr(images), None, None, None, ptr(images), stream_ptr()) == 0
        assert s.stats()[3] == 0
        assert L().vga_hps_read_device_v(r._h, ptr(images), ptr(images), None, None, None, None, stream_ptr()) == 0
        assert r.stats()[3] == 0
        assert L().vga_hps_write_device_v(s._h, None, None, None, None, None, None, None) == 0
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
        a = WriteSet()                                                 # (created under the mode: its tables are poisoned first)
        try:
            images = a.run(a.inputs(), a.images(value ^ 0x3C))
            torch().cuda.synchronize()
            a.check(images, False, ("poison", value), fill=value ^ 0x3C)
        finally:
            a.close()
        files, parsed = written()
        r = HpsFileSet.from_infos(parsed)
        try:
            packed = packed_images(r, files, r.totals.image_bytes, value)
            rows = torch().full((r.totals.adpcm_bytes,), value ^ 0x3C, dtype=torch().uint8, device="cuda")
            r.read(dev(packed), rows)
            torch().cuda.synchronize()
            check_rows(r, host(rows), files, parsed, ("poison", value), fill=value ^ 0x3C)
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
    a = WriteSet()
    files, parsed = written()
    r = HpsFileSet.from_infos(parsed)
    try:
        (S,) = some_streams(1)
        b = a.inputs()
        source, source_pcm = b["adpcm"], b["pcm"]
        d_packed = dev(packed_images(r, files, r.totals.image_bytes))
        with t.cuda.stream(S):
            for busy in (False, True):                                 # (warm first: every kernel has run once)
                b["adpcm"], b["pcm"] = t.zeros_like(source), t.zeros_like(source_pcm)
                d_images = t.zeros_like(d_packed)
                images, rows = a.images(), t.full((r.totals.adpcm_bytes,), JUNK, dtype=t.uint8, device="cuda")
                S.synchronize()
                if busy:
                    t.cuda._sleep(cycles)
                b["adpcm"].copy_(source, non_blocking=True)            # the inputs arrive behind the delay
                b["pcm"].copy_(source_pcm, non_blocking=True)
                d_images.copy_(d_packed, non_blocking=True)
                a.run(b, images, stream=S)
                r.read(d_images, rows, stream=S)
                if busy:
                    assert not S.query(), "the caller's stream was idle when the calls returned (they waited for it)"
        S.synchronize()
        a.check(images, False, "busy stream")
        check_rows(r, host(rows), files, parsed, "busy stream")
    finally:
        r.close()
        a.close()


def test_two_calls_on_two_streams():
    """one object, two streams"""
    t = torch()
    a = WriteSet()
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
    a = WriteSet()
    files, parsed = written()
    r = HpsFileSet.from_infos(parsed)
    try:
        b, images = a.inputs(), a.images()
        rows = t.full((a.t.adpcm_bytes + EXTRA,), JUNK, dtype=t.uint8, device="cuda")
        A, K, P, I, R = ptr(b["adpcm"]), ptr(b["coefs"]), ptr(b["pcm"]), ptr(images), ptr(rows)
        write, read = L().vga_hps_write_device_v, L().vga_hps_read_device_v
        assert write(a.s._h, A + 8, K, None, None, None, I, None) == ARG
        assert write(a.s._h, A, K, None, None, P + 8, I, None) == ARG
        assert write(a.s._h, A, K, None, None, None, I + 8, None) == ARG
        assert write(a.s._h, None, K, None, None, None, I, None) == ARG and write(a.s._h, A, None, None, None, None, I, None) == ARG
        assert write(a.s._h, A, K, None, None, None, None, None) == ARG
        assert write(r._h, A, K, None, None, None, I, None) == OP           # a set for reading
        assert read(a.s._h, I, R, None, None, None, None, None) == OP       # a set for writing
        assert read(r._h, I + 8, R, None, None, None, None, None) == ARG and read(r._h, I, R + 8, None, None, None, None, None) == ARG
        assert read(r._h, None, R, None, None, None, None, None) == ARG and read(r._h, I, None, None, None, None, None, None) == ARG
        assert a.s.stats()[3] == 0
        assert L().vga_hps_files_gc_files(r._h, (_lib.GcFileC * r.files)()) == OP
        t.cuda.synchronize()
        assert np.all(host(images) == JUNK) and np.all(host(rows) == JUNK)
        # exactly at the minimum: buffers of the totals' sizes
        exact, exact_pcm = b["adpcm"][:a.t.adpcm_bytes].clone(), b["pcm"][:a.t.pcm_samples].clone()
        out = t.full((a.t.image_bytes,), JUNK, dtype=t.uint8, device="cuda")
        assert write(a.s._h, ptr(exact), K, ptr(b["gain"]), ptr(b["start"]), ptr(exact_pcm), ptr(out), None) == 0
        t.cuda.synchronize()
        a.check(out, False, "at the minimum")
    finally:
        r.close()
        a.close()


# ---------------------------------------------------------------- 8. the Python mirror
def test_write_files_and_read_files_are_the_mirrors():
    """hps.write_files -- upload, coefficients, encode, align and assemble on the device, one download -- gives per file what
    HpsWriter().GetFile(GcAdpcmFormat().EncodeFromPcm16(file)) returns, and hps.read_files what HpsReader().ReadFormat returns, the
    PCM what its ToPcm16 gives"""
    from vgaudio_amd import gcadpcm, hps
    files = pcm_files(SHAPES)
    got = hps.write_files(files)
    writer = hps.HpsWriter()
    for k, f in enumerate(files):
        assert got[k] == writer.GetFile(gcadpcm.GcAdpcmFormat().EncodeFromPcm16(f)), ("file", k)
    assert hps.write_files([]) == [] and hps.read_files([]) == []
    formats, pcm = hps.read_files(got, pcm=True)
    for k, (image, fmt) in enumerate(zip(got, formats)):
        want = hps.HpsReader().ReadFormat(image)
        assert (fmt.ChannelCount, fmt.SampleRate, fmt.SampleCount, fmt.Looping) == (want.ChannelCount, want.SampleRate, want.SampleCount, want.Looping)
        decoded = want.ToPcm16()
        for c in range(want.ChannelCount):
            assert np.array_equal(fmt.Channels[c].GetAdpcmAudio(), want.Channels[c].GetAdpcmAudio()), ("file", k, "channel", c)
            assert np.array_equal(fmt.Channels[c].Coefs, want.Channels[c].Coefs)
            assert np.array_equal(pcm[k][c], np.asarray(decoded.Channels[c], np.int16)[:want.SampleCount]), ("file", k, "pcm", c)

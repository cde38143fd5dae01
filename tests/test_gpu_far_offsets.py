"""The device calls with their rows, images and offsets more than 2, 4 and 8 GiB apart.

Every entry point takes int64_t pitches or offsets; the other tests keep a batch within a few MB (test_gpu_full_size.py
crosses 4 GiB for five calls, at full workload size).  Three parts, and a CPU census over them:

A. calls with a pitch (FAR_PITCH).  The smallest batch test_gpu_device_layouts.py / test_gpu_container_layouts.py use for a
call lies in a FarBuffer (far_memory.py) with its rows D bytes apart:

    D = 2^31 + a, three rows, the batch 2^31 bytes into its allocation: row 1 lies past 2^31, row 2 past 2^32, and an offset
                  that went through a signed 32-bit value still falls inside the allocation
    D = 2^32 + a, two rows: an offset cut to 32 bits is a (row 0's neighbourhood)
    D = 2^33 + a, two rows: the same for a count of dwords or samples

a is the smallest non-zero residue the call's contract allows, so row 1's true offset and its low 32 bits always differ
(test_row_1_never_lies_where_its_low_32_bits_point).  Inputs and outputs are far at once (two allocations of up to 8 GiB + a
row, under the 20 GiB a test may take).  Expected bytes are the oracle's, through the cached cases of
test_gpu_device_layouts.py; every row is compared byte for byte, an input allocation may not change at all and an output
allocation only in its rows (plus SLOP bytes behind a row where the header does not promise that they are left alone: a
kernel may finish its last vector).  A wrong offset therefore shows as wrong bytes in a row or as changed junk, not as a fault.

vga_hca_decode_device at 2^33: before its fix the scan kernel formed a stream's readable dwords, frames_pitch / 4 less the
frame's own, in an int.  With a pitch of 8 GiB and a little that is negative for each stream's frame 0 (2^31 + 4 dwords; the
later frames subtract enough to fit), every read of that frame is clamped to dword limit - 1 -- 8 GiB IN FRONT of the stream --
and the scan sees one dword repeated where the frame is.  Measured on that code with frames_pitch = 2^33 + 16, two streams of
one channel and seven frames, the batch 2^33 bytes into a 16 GiB allocation of 0xA7 (so that the read stays inside it): rc 0,
status word 3 (bad sync | bad scale factor), the first 1024 samples of both streams wrong (up to 11053 and 22700 off), every
later sample right, no input byte changed.  With the count clamped as the packed branch always clamped it: status 0, every
sample the oracle's.  Pitches from 2^34 on wrapped to small positive counts and would have cut frames short instead.

The container calls run in the shapes of SHAPES (rows are files x channels, so both the row pitch and the file pitch are
far); a call with three or four pitched buffers takes them in turn where all at once would pass 20 GiB.

B. sets made at the caller's offsets (FAR_OFFSETS): six small files of the existing *_files_cases.py at 0, under 2^31, across
2^32, behind it, across 2^33 and behind that (far_spots), written from far rows and read from far images, against the
references of the near tests, bad-CRC counts and per-channel arrays included.

C. objects that pack their own buffers (FAR_PACKED): one ballast channel of about 2^22 samples replicated until groups of
short probes lie behind 2^31 and 2^32 bytes of each packed buffer; see "packed objects" below.  48 GiB a test at most.

test_every_device_entry_point_is_in_exactly_one_table holds every device call of the four header groups to one of FAR_PITCH,
FAR_OFFSETS, FAR_PACKED and NO_DISTANCE and the named test to making the call (a chain to making every call of its stages:
CHAIN_STAGES).  A test skips only when the device has less free memory than it is about to use.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import far_memory as fm
import test_gpu_device_layouts as lay

GIB = 1 << 30
SLOP = 64
# name: (bytes between rows less a, rows, bytes from the allocation's start to the batch)
DISTANCES = {"2^31": (1 << 31, 3, 1 << 31), "2^32": (1 << 32, 2, 256), "2^33": (1 << 33, 2, 256)}
DIST = list(DISTANCES)
TAIL = 4096                 # behind the last row: a clamped over-read stays inside the allocation

# call: (test, the residue a in bytes per far buffer)
FAR_PITCH = {
    "vga_gcadpcm_coefs_device": ("test_gc_coefs", dict(pcm=4)),
    "vga_gcadpcm_encode_device": ("test_gc_encode", dict(pcm=4, adpcm=8)),
    "vga_gcadpcm_decode_device": ("test_gc_decode", dict(adpcm=8, pcm=4)),
    "vga_adx_encode_device": ("test_adx_encode", dict(pcm=2, adx=2)),
    "vga_adx_decode_device": ("test_adx_decode", dict(adx=1, pcm=2)),
    "vga_hca_encode_device": ("test_hca_encode", dict(pcm=2, frames=2)),
    "vga_hca_decode_device": ("test_hca_decode", dict(frames=4, pcm=2)),
    "vga_adx_crypt_device": ("test_adx_crypt", dict(audio=1)),
    "vga_adx_find_key_device": ("test_adx_find_key", dict(audio=1)),
    "vga_hca_crypt_device": ("test_hca_crypt", dict(frames=1)),
    "vga_hca_byte_position_counts_device": ("test_hca_byte_position_counts", dict(frames=1)),
    # the container calls: rows at any byte; several images a writer fills lie a multiple of 16 apart
    "vga_gcadpcm_build_channels_device": ("test_gc_build_channels", dict(adpcm=8, adpcm_out=8, pcm=4, seek=2)),
    "vga_dsp_write_device": ("test_dsp_write", dict(adpcm=8)),
    "vga_dsp_read_device": ("test_dsp_read", dict(files=1, rows=1)),
    "vga_nwstm_write_device": ("test_nwstm_write", dict(adpcm=1, files=16)),
    "vga_nwstm_read_device": ("test_nwstm_read", dict(files=1, rows=1)),
    "vga_hps_write_device": ("test_hps_write", dict(adpcm=1, pcm=2, files=16)),
    "vga_hps_read_device": ("test_hps_read", dict(files=1, rows=1)),
    "vga_idsp_write_device": ("test_idsp_write", dict(adpcm=1, files=16)),
    "vga_idsp_read_device": ("test_idsp_read", dict(files=1, rows=1)),
    "vga_genh_read_device": ("test_genh_read", dict(files=1, rows=1)),
    "vga_adx_write_device": ("test_adx_write", dict(audio=1)),
    "vga_adx_read_device": ("test_adx_read", dict(files=1, rows=1)),
    "vga_hca_write_device": ("test_hca_write", dict(frames=1, files=1)),
    "vga_hca_read_device": ("test_hca_read", dict(files=1, frames=4)),
    "vga_synth_pcm16_device": ("test_synth_pcm16", dict(pcm=2)),
    "vga_wave_write_pcm16_device": ("test_wave_pcm16", dict(pcm=2)),
    "vga_wave_deinterleave_pcm16_device": ("test_wave_pcm16", dict(pcm=2)),
    # include/vgaudio_hip_pcm.h
    "vga_pcm8_encode_device": ("test_pcm8_encode", dict(pcm=2, bytes=1)),
    "vga_pcm8_decode_device": ("test_pcm8_decode", dict(bytes=1, pcm=2)),
    "vga_nwstm_pcm_write_device": ("test_nwstm_pcm_write", dict(rows=1, files=16)),
    "vga_nwstm_pcm_read_device": ("test_nwstm_pcm_read", dict(files=1, rows=1)),
    "vga_wave_write_pcm8_device": ("test_wave_pcm8", dict(rows=1)),
    "vga_wave_deinterleave_pcm8_device": ("test_wave_pcm8", dict(rows=1)),
}


def _residue(call, buf):
    return FAR_PITCH[call][1][buf]


# calls of a set (or bank) made at the caller's offsets -> the test that puts six files around 2^31, 2^32 and 2^33
FAR_OFFSETS = {
    "vga_adx_write_device_v": "test_adx_files_write_from_far_rows", "vga_adx_read_device_v": "test_adx_files_read_from_far_images",
    "vga_hca_write_device_v": "test_hca_files_write_from_far_frames", "vga_hca_read_device_v": "test_hca_files_read_far",
    "vga_dsp_read_device_v": "test_dsp_files_read_from_far_images", "vga_nwstm_read_device_v": "test_nw_files_read_from_far_images",
    "vga_nwwav_bank_read_device": "test_nwwav_bank_read_from_far_files",
}
# calls on objects that pack their own buffers -> the chain test that pushes probes past 2^31 and 2^32 with ballast.  The calls
# of FAR_OFFSETS' sets run in the chains too, over the packed rows (CHAIN_STAGES: the stages of a chain and their calls)
FAR_PACKED = {
    "vga_gcadpcm_coefs_device_v": "test_gc_packed_chain", "vga_gcadpcm_encode_device_v": "test_gc_packed_chain",
    "vga_gcadpcm_decode_device_v": "test_gc_packed_chain",
    "vga_gcadpcm_build_channels_device_v": "test_gc_packed_chain", "vga_dsp_write_device_v": "test_gc_packed_chain",
    "vga_gcadpcm_align_channels_device_v": "test_gc_packed_chain", "vga_nwstm_write_device_v": "test_gc_packed_chain",
    "vga_adx_encode_device_v": "test_adx_packed_chain", "vga_adx_decode_device_v": "test_adx_packed_chain",
    "vga_hca_encode_device_v": "test_hca_packed_chain", "vga_hca_decode_device_v": "test_hca_packed_chain",
}
# chain test -> the functions that are its stages (the test's own body first) and every call the chain must make in them
CHAIN_STAGES = {
    "test_gc_packed_chain": (("test_gc_packed_chain", "_gc_files_over_the_rows", "_nw_files_over_the_rows"),
                             ("vga_gcadpcm_coefs_device_v", "vga_gcadpcm_encode_device_v", "vga_gcadpcm_decode_device_v",
                              "vga_gcadpcm_build_channels_device_v", "vga_dsp_write_device_v", "vga_dsp_read_device_v",
                              "vga_gcadpcm_align_channels_device_v", "vga_nwstm_write_device_v", "vga_nwstm_read_device_v")),
    "test_adx_packed_chain": (("test_adx_packed_chain", "_adx_files_over_the_rows"),
                              ("vga_adx_encode_device_v", "vga_adx_write_device_v", "vga_adx_read_device_v", "vga_adx_decode_device_v")),
    "test_hca_packed_chain": (("test_hca_packed_chain", "_hca_files_over_the_frames"),
                              ("vga_hca_encode_device_v", "vga_hca_write_device_v", "vga_hca_read_device_v", "vga_hca_decode_device_v")),
}
# calls in which no distance between two things enters an address
NO_DISTANCE = {
    "vga_hca_find_key_device": "no pitch: the frames of one stream, back to back from d_frames",
}


def own_text():
    return open(os.path.abspath(__file__)).read()


def all_device_entry_points():
    """every vga_*_device / vga_*_device_v function of vgaudio_hip.h, vgaudio_hip_pcm.h, vgaudio_hip_nwwav.h and vgaudio_hip/*.h"""
    cl = _cl()
    names = set(lay.header_device_entry_points()) | cl._declared("vgaudio_hip_pcm.h") | cl._declared("vgaudio_hip_nwwav.h")
    for f in sorted(os.listdir(os.path.join(lay.ROOT, "include", "vgaudio_hip"))):
        names |= cl._declared(os.path.join("vgaudio_hip", f))
    return names


def test_every_device_entry_point_is_in_exactly_one_table():
    declared = all_device_entry_points()
    assert len(declared) >= 53, len(declared)
    tables = (FAR_PITCH, FAR_OFFSETS, FAR_PACKED, NO_DISTANCE)
    listed = [name for t in tables for name in t]
    assert len(listed) == len(set(listed)), sorted(n for n in set(listed) if listed.count(n) > 1)
    assert set(listed) == declared, (sorted(declared - set(listed)), sorted(set(listed) - declared))
    assert all(NO_DISTANCE.values())
    own = own_text()
    for name, test in FAR_OFFSETS.items():                       # the named test itself makes the call
        body = lay._function_body(own, test)
        assert body, (name, test)
        assert re.search(r"\b" + name + r"\(", body), (name, test)
    assert set(FAR_PACKED.values()) == set(CHAIN_STAGES)
    for test, (stages, calls) in CHAIN_STAGES.items():           # a chain: the test calls every stage, the stages make the calls
        bodies = [lay._function_body(own, f) for f in stages]
        assert all(bodies) and stages[0] == test, (test, stages)
        assert all(re.search(r"\b" + f + r"\(", bodies[0]) for f in stages[1:]), (test, "does not call its stages")
        assert {n for n, t in FAR_PACKED.items() if t == test} <= set(calls)
        for name in calls:
            assert name in declared and any(re.search(r"\b" + name + r"\(", b) for b in bodies), (test, name)


# ====================================================================== CPU
def test_far_tables_name_tests_that_make_the_call():
    own = own_text()
    for name, (test, residues) in FAR_PITCH.items():
        body = lay._function_body(own, test)
        assert body, (name, test)
        assert re.search(r"\b" + name + r"\(", body), (name, test)
        assert re.search(r'parametrize\("dist(?:,nch,nf)?", (?:DIST|SHAPES)\)\n(?:@.*\n)*def ' + test + r"\(", own), \
            (name, "not run at the three distances")
        assert residues and all(0 < a < 256 for a in residues.values())


def test_row_1_never_lies_where_its_low_32_bits_point():
    """what a reviewer checks: at every distance and residue row 1's offset from the batch's base differs from that offset
    cut to 32 bits and from it read as a signed 32-bit value, and both wrong places lie inside the allocation"""
    for name, (d0, rows, base) in DISTANCES.items():
        for call, (_, residues) in FAR_PITCH.items():
            for a in residues.values():
                extent = base + (rows - 1) * (d0 + a) + TAIL
                for r in range(1, rows):
                    true = r * (d0 + a)
                    cut = true & 0xFFFFFFFF
                    signed = cut - (1 << 32) if cut >= 1 << 31 else cut
                    assert signed != true and (cut != true or r < rows - 1), (name, call, a, r)
                    assert 0 <= base + cut < extent and 0 <= base + signed < extent, (name, call, a, r)
        assert (rows - 1) * d0 >= 1 << 32 or name != "2^31"


def test_the_residues_are_the_contract_minimum():
    """a is the least the call accepts: GC PCM pitch even and base 4-byte aligned, GC ADPCM multiples of 8 (vgaudio_hip.h
    "device-resident GC-ADPCM"), ADX and HCA PCM any sample, ADX and HCA encoder output even, HCA decoder input a multiple of
    4, everything else any byte"""
    r = {c: v[1] for c, v in FAR_PITCH.items()}
    assert r["vga_gcadpcm_coefs_device"]["pcm"] == r["vga_gcadpcm_encode_device"]["pcm"] == r["vga_gcadpcm_decode_device"]["pcm"] == 4
    assert r["vga_gcadpcm_encode_device"]["adpcm"] == r["vga_gcadpcm_decode_device"]["adpcm"] == 8
    assert r["vga_adx_encode_device"] == dict(pcm=2, adx=2) and r["vga_adx_decode_device"] == dict(adx=1, pcm=2)
    assert r["vga_hca_encode_device"] == dict(pcm=2, frames=2) and r["vga_hca_decode_device"] == dict(frames=4, pcm=2)


# ====================================================================== helpers (GPU only below this line)
_torch, _L, _po, _stream, _ok, _eq = lay._torch, lay._L, lay._po, lay._stream, lay._ok, lay._eq


class FarRows:
    """`units` far rows in a FarBuffer of their own, each `sub` rows of `width` elements `sub_pitch` elements apart (an HCA
    stream's channels; sub = 1 elsewhere).  data: one array per row, or None for an output.  .ptr and .pitch (elements) are
    what the call takes."""

    def __init__(self, dist, a, width, dtype, data=None, sub=1, sub_pitch=0, slop=0, units=None, base=None):
        d0, self.units, own_base = DISTANCES[dist]
        self.units = units or self.units
        base = own_base if base is None else base
        self.dtype = np.dtype(dtype)
        isz = self.dtype.itemsize
        assert (d0 + a) % isz == 0
        self.pitch = (d0 + a) // isz
        self.sub, self.width, self.slop = sub, width, slop
        self.offs = [base + u * (d0 + a) + s * sub_pitch * isz for u in range(self.units) for s in range(sub)]
        extent = lay._round_up(self.offs[-1] + width * isz + TAIL, 256)
        fm.need(extent)
        self.buf = fm.FarBuffer(extent)
        self.ptr = self.buf.ptr + base
        self.data = None
        if data is not None:
            self.data = [np.ascontiguousarray(r, dtype=self.dtype) for r in data]
            assert len(self.data) == len(self.offs) and all(len(r) == width for r in self.data)
            for o, r in zip(self.offs, self.data):
                self.buf.put(o, r)

    def rows(self):
        return np.stack([self.buf.get(o, self.width * self.dtype.itemsize, self.dtype) for o in self.offs])

    def clean(self, what):
        """an input: its rows as they were; both: every byte outside the rows (and their slop) still the fill"""
        if self.data is not None and not self.slop:
            _eq(self.rows(), np.stack(self.data), what + " (input, after the call)")
        first = self.buf.untouched([(o, self.width * self.dtype.itemsize + self.slop) for o in self.offs])
        assert first is None, (f"{what}: {self.buf.changed} bytes outside the rows changed, the first {first - (self.ptr - self.buf.ptr)} "
                               f"bytes from the base (rows {self.pitch * self.dtype.itemsize} bytes apart)")


def _status():
    return _torch().zeros(4, dtype=_torch().int32, device="cuda")


def _done(*rows):
    fm.release(*[r.buf for r in rows if r is not None])


# ====================================================================== the helper itself
@pytest.mark.gpu
def test_far_buffer_sees_one_stray_byte_past_4_gib():
    torch = _torch()
    fm.need(5 * GIB)
    b = fm.FarBuffer(4 * GIB + 4096)
    try:
        w = [b.put(100, np.arange(50, dtype=np.uint8)), b.put(4 * GIB + 7, np.arange(9, dtype=np.int16))]
        assert w == [(100, 50), (4 * GIB + 7, 18)]
        assert b.untouched(w) is None and b.changed == 0
        assert np.array_equal(b.get(4 * GIB + 7, 18, np.int16), np.arange(9, dtype=np.int16))
        assert b.get(7, 18).tolist() == [fm.FILL] * 18                     # not where the low 32 bits point
        b.t[4 * GIB + 25] = 0                                            # the byte behind the second window
        b.t[4 * GIB + 3000] = 1
        assert b.untouched(w) == 4 * GIB + 25 and b.changed == 2
        assert b.untouched(w + [(4 * GIB + 25, 1)]) == 4 * GIB + 3000 and b.changed == 1
        b.t[99] = 3
        assert b.untouched(w) == 99 and b.changed == 3
        torch.cuda.synchronize()
    finally:
        fm.release(b)


# ====================================================================== GC-ADPCM
@pytest.mark.gpu
@pytest.mark.parametrize("dist", DIST)
def test_gc_coefs(dist):
    torch = _torch()
    L = _L()
    n = lay._gc_n()
    d_pcm = d_coefs = None
    try:
        nch = DISTANCES[dist][1]
        d_pcm = FarRows(dist, _residue("vga_gcadpcm_coefs_device", "pcm"), n, np.int16, data=lay._gc().cases()[0][:nch])
        d_coefs = lay.place((1, nch * 16), nch * 16, 0, np.int16)
        ws = torch.empty(max(L.vga_gcadpcm_coefs_workspace_bytes(nch, n), 16), dtype=torch.uint8, device="cuda")
        _ok(L.vga_gcadpcm_coefs_device(d_pcm.ptr, d_pcm.pitch, nch, n, d_coefs.ptr, ws.data_ptr(), ws.numel(), _stream()))
        torch.cuda.synchronize()
        _eq(d_coefs.rows().reshape(nch, 16), lay._gc_own_coefs()[:nch], "coefs")
        d_coefs.kept("coefs", padding=True)
        d_pcm.clean("pcm")
    finally:
        _done(d_pcm)


@pytest.mark.gpu
@pytest.mark.parametrize("dist", DIST)
def test_gc_encode(dist):
    torch = _torch()
    L = _L()
    n, nb = lay._gc_n(), lay._gc_nb()
    pcm, coefs, h1, h2, want, _ = lay._gc().cases()
    nch = DISTANCES[dist][1]
    made = []
    try:
        d_pcm = FarRows(dist, _residue("vga_gcadpcm_encode_device", "pcm"), n, np.int16, data=pcm[:nch])
        made.append(d_pcm)
        d_out = FarRows(dist, _residue("vga_gcadpcm_encode_device", "adpcm"), nb, np.uint8, slop=SLOP)
        made.append(d_out)
        d_coefs, d_h1, d_h2 = lay._up(coefs[:nch]), lay._up(h1[:nch]), lay._up(h2[:nch])
        _ok(L.vga_gcadpcm_encode_device(d_pcm.ptr, d_pcm.pitch, nch, n, d_coefs.data_ptr(), d_h1.data_ptr(), d_h2.data_ptr(), d_out.ptr,
                                        d_out.pitch, _stream()))
        torch.cuda.synchronize()
        _eq(d_out.rows(), want[:nch], "adpcm")
        d_out.clean("adpcm")
        d_pcm.clean("pcm")
    finally:
        _done(*made)


@pytest.mark.gpu
@pytest.mark.parametrize("dist", DIST)
def test_gc_decode(dist):
    torch = _torch()
    L = _L()
    n, nb = lay._gc_n(), lay._gc_nb()
    pcm, coefs, h1, h2, want, end = lay._gc().cases()
    nch = DISTANCES[dist][1]
    made = []
    try:
        d_in = FarRows(dist, _residue("vga_gcadpcm_decode_device", "adpcm"), nb, np.uint8, data=want[:nch])
        made.append(d_in)
        d_out = FarRows(dist, _residue("vga_gcadpcm_decode_device", "pcm"), n, np.int16)       # the columns >= n stay: no slop
        made.append(d_out)
        d_coefs, d_h1, d_h2 = lay._up(coefs[:nch]), lay._up(h1[:nch]), lay._up(h2[:nch])
        status = _status()
        _ok(L.vga_gcadpcm_decode_device(d_in.ptr, d_in.pitch, d_coefs.data_ptr(), nch, n, d_h1.data_ptr(), d_h2.data_ptr(), d_out.ptr,
                                        d_out.pitch, status.data_ptr(), _stream()))
        torch.cuda.synchronize()
        assert status.cpu().numpy().tolist() == [0, 0, 0, 0]
        _eq(d_out.rows(), lay._gc_decoded()[:nch], "pcm")
        d_out.clean("pcm")
        d_in.clean("adpcm")
    finally:
        _done(*made)


# ====================================================================== ADX
# the contract minimum sends every call to the general kernel (one lane per channel); `pieces` adds 16 bytes to the residue
# of both buffers, the layout the time-piece kernels take, so that their addressing is far as well
ADX_FORMS = ["min", "pieces"]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ADX_FORMS)
@pytest.mark.parametrize("dist", DIST)
def test_adx_encode(dist, form):
    torch = _torch()
    L = _L()
    nch = DISTANCES[dist][1]
    for k in (0, 4):                                             # 18-byte frames, 34-byte frames (always the general kernel)
        kw = lay.ADX_SETS[k]
        pcm, want, whist, _ = lay._adx_case(k)
        p, _ = lay._adx_params(**kw)
        nb = want.shape[1]
        made = []
        try:
            a_pcm, a_adx = (16, 16) if form == "pieces" else (_residue("vga_adx_encode_device", "pcm"), _residue("vga_adx_encode_device", "adx"))
            d_pcm = FarRows(dist, a_pcm, lay.ADX_N, np.int16, data=pcm[:nch])
            made.append(d_pcm)
            d_out = FarRows(dist, a_adx, nb, np.uint8, slop=SLOP)
            made.append(d_out)
            d_hist = lay.place((1, nch), nch, 0, np.int16)
            _ok(L.vga_adx_encode_device(d_pcm.ptr, d_pcm.pitch, nch, lay.ADX_N, C.byref(p), d_out.ptr, d_out.pitch, d_hist.ptr, _stream()))
            path = lay._adx_path()[0]
            torch.cuda.synchronize()
            _eq(d_out.rows(), want[:nch], f"adx {kw}")
            _eq(d_hist.rows().reshape(-1), whist[:nch], f"history_out {kw}")
            d_hist.kept("history_out", padding=True)
            d_out.clean(f"adx {kw}")
            d_pcm.clean(f"pcm {kw}")
            assert path == (lay.PATH_PIECES if form == "pieces" and k == 0 else lay.PATH_GENERAL), (kw, form, path)
        finally:
            _done(*made)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ADX_FORMS)
@pytest.mark.parametrize("dist", DIST)
def test_adx_decode(dist, form):
    torch = _torch()
    L = _L()
    nch = DISTANCES[dist][1]
    for k in (0, 4):
        kw = lay.ADX_SETS[k]
        _, adx, _, want = lay._adx_case(k)
        p, _ = lay._adx_params(**kw)
        nb = adx.shape[1]
        made = []
        try:
            a_adx, a_pcm = (16, 16) if form == "pieces" else (_residue("vga_adx_decode_device", "adx"), _residue("vga_adx_decode_device", "pcm"))
            d_in = FarRows(dist, a_adx, nb, np.uint8, data=adx[:nch])
            made.append(d_in)
            d_out = FarRows(dist, a_pcm, lay.ADX_N, np.int16, slop=SLOP)
            made.append(d_out)
            status = _status()
            _ok(L.vga_adx_decode_device(d_in.ptr, d_in.pitch, nb, nch, lay.ADX_N, C.byref(p), d_out.ptr, d_out.pitch, status.data_ptr(),
                                        _stream()))
            path = lay._adx_path()[1]
            torch.cuda.synchronize()
            assert status.cpu().numpy().tolist() == [0, 0, 0, 0], kw
            _eq(d_out.rows(), want[:nch], f"pcm {kw}")
            d_out.clean(f"pcm {kw}")
            d_in.clean(f"adx {kw}")
            assert path == (lay.PATH_PIECES if form == "pieces" and k == 0 else lay.PATH_GENERAL), (kw, form, path)
        finally:
            _done(*made)


# ====================================================================== HCA
HCA_FAR_NCH = [1, 6]        # the wave encoder and the workgroup encoder; streams are the far rows, channels follow each other


@pytest.mark.gpu
@pytest.mark.parametrize("nch", HCA_FAR_NCH)
@pytest.mark.parametrize("dist", DIST)
def test_hca_encode(dist, nch):
    torch = _torch()
    L = _L()
    ns = DISTANCES[dist][1]
    pcm, info, want, _ = lay._hca_case(nch)
    fb = want.shape[1]
    cp = lay.HCA_N | 1
    made = []
    try:
        d_pcm = FarRows(dist, _residue("vga_hca_encode_device", "pcm"), lay.HCA_N, np.int16, data=pcm[:ns].reshape(ns * nch, lay.HCA_N),
                        sub=nch, sub_pitch=cp)
        made.append(d_pcm)
        d_out = FarRows(dist, _residue("vga_hca_encode_device", "frames"), fb, np.uint8, slop=SLOP)
        made.append(d_out)
        status = _status()
        _ok(L.vga_hca_encode_device(d_pcm.ptr, d_pcm.pitch, cp, ns, lay.HCA_N, C.byref(info), d_out.ptr, d_out.pitch, status.data_ptr(),
                                    _stream()))
        torch.cuda.synchronize()
        assert status.cpu().numpy().tolist() == [0, 0, 0, 0]
        _eq(d_out.rows(), want[:ns], "frames")
        d_out.clean("frames")
        d_pcm.clean("pcm")
    finally:
        _done(*made)


@pytest.mark.gpu
@pytest.mark.parametrize("nch", HCA_FAR_NCH)
@pytest.mark.parametrize("dist", DIST)
def test_hca_decode(dist, nch):
    """2^33: the case the scan kernel's 32-bit count of readable dwords got wrong (the module's docstring has what it gave).
    With that count in an int, frame 0 of every stream reads the dword 2^33 - 12 bytes IN FRONT of its stream, so at 2^33 the
    batch of frames lies 2^33 bytes into its allocation: the code as it was returns wrong samples here, not a fault.  That
    allocation is 16 GiB, so at 2^33 the two sides are far in turn (frames far and PCM near, then the other way round)"""
    torch = _torch()
    L = _L()
    ns = DISTANCES[dist][1]
    _, info, frames, want = lay._hca_case(nch)
    fb, n = frames.shape[1], want.shape[2]
    cp = n | 1
    for far_in, far_out in ([(True, False), (False, True)] if dist == "2^33" else [(True, True)]):
        made = []
        try:
            if far_in:
                d_in = FarRows(dist, _residue("vga_hca_decode_device", "frames"), fb, np.uint8, data=frames[:ns],
                               base=1 << 33 if dist == "2^33" else None)
                made.append(d_in)
            else:
                d_in = lay.place(frames[:ns], lay._round_up(fb + 8, 16), 0, np.uint8)
            if far_out:
                d_out = FarRows(dist, _residue("vga_hca_decode_device", "pcm"), n, np.int16, sub=nch, sub_pitch=cp, slop=SLOP)
                made.append(d_out)
                sp = d_out.pitch
            else:
                sp = nch * cp + 3
                d_out = lay.place((ns * nch, n), cp, 0, np.int16, offsets=[s * sp + c * cp for s in range(ns) for c in range(nch)],
                                  extent=ns * sp)
            wsb = L.vga_hca_decode_workspace_bytes(C.byref(info), ns)
            ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
            status = _status()
            _ok(L.vga_hca_decode_device(C.byref(info), d_in.ptr, d_in.pitch, ns, d_out.ptr, sp, cp, ws.data_ptr(), wsb,
                                        status.data_ptr(), _stream()))
            torch.cuda.synchronize()
            assert status.cpu().numpy().tolist() == [0, 0, 0, 0], (far_in, far_out)
            _eq(d_out.rows().reshape(ns, nch, n), want[:ns], f"pcm (frames far: {far_in}, pcm far: {far_out})")
            if far_out:
                d_out.clean("pcm")
            else:
                d_out.kept("pcm")
            _checked(d_in, "frames")
        finally:
            _done(*made)


# ====================================================================== encryption
@pytest.mark.gpu
@pytest.mark.parametrize("etype", [8, 9])
@pytest.mark.parametrize("dist", DIST)
def test_adx_crypt(dist, etype):
    torch = _torch()
    po = _po()
    nch, frames = DISTANCES[dist][1], 301
    audio = np.random.default_rng(170).integers(0, 256, (nch, 18 * frames)).astype(np.uint8)
    audio[:, 18 * 7:18 * 8] = 0
    key = lay._adx_keys()[3]
    want = np.stack(po.adx_crypt(list(audio), lay._okey(key), etype))
    d = None
    try:
        d = FarRows(dist, _residue("vga_adx_crypt_device", "audio"), 18 * frames, np.uint8, data=audio)
        d.data = None                                            # in place: an output from here on
        _ok(_L().vga_adx_crypt_device(d.ptr, d.pitch, 18 * frames, nch, C.byref(key), etype, 18, _stream()))
        torch.cuda.synchronize()
        _eq(d.rows(), want, "audio")
        d.clean("audio")
    finally:
        _done(d)


@pytest.mark.gpu
@pytest.mark.parametrize("dist", DIST)
def test_adx_find_key(dist):
    po = _po()
    nch, n = DISTANCES[dist][1], 32 * 800
    pcm = po.synth_generate(nch, n, first_channel=77)
    audio, _ = po.adx_encode_batch(pcm, po.adx_params())
    keys = lay._adx_keys()
    target = 4
    enc = np.stack(po.adx_crypt(list(audio), lay._okey(keys[target]), 8))
    want = next(i for i in range(len(keys)) if po.adx_test_key(list(enc), lay._okey(keys[i]), 8))
    assert want == target
    nb = enc.shape[1]
    d = None
    try:
        d = FarRows(dist, _residue("vga_adx_find_key_device", "audio"), nb, np.uint8, data=enc)
        idx = C.c_int(-7)
        _ok(_L().vga_adx_find_key_device(d.ptr, d.pitch, nb, nch, 8, 18, keys, len(keys), C.byref(idx), _stream()))
        assert idx.value == want
        d.clean("audio")
    finally:
        _done(d)


@pytest.mark.gpu
@pytest.mark.parametrize("dist", DIST)
def test_hca_crypt(dist):
    from vgaudio_amd import _lib
    torch = _torch()
    po = _po()
    ns, fc, fs = DISTANCES[dist][1], 37, 682
    frames = np.random.default_rng(180).integers(0, 256, (ns, fc * fs)).astype(np.uint8)
    rc, dec, enc = po.hca_key_tables(56, 123456789)
    want = np.stack([po.hca_crypt(frames[s], fs, enc) for s in range(ns)])
    d = None
    try:
        d = FarRows(dist, _residue("vga_hca_crypt_device", "frames"), fc * fs, np.uint8, data=frames)
        d.data = None
        _ok(_L().vga_hca_crypt_device(d.ptr, d.pitch, ns, fc, fs, enc.ctypes.data_as(_lib.u8p), _stream()))
        torch.cuda.synchronize()
        _eq(d.rows(), want, "frames")
        d.clean("frames")
    finally:
        _done(d)


@pytest.mark.gpu
@pytest.mark.parametrize("dist", DIST)
def test_hca_byte_position_counts(dist):
    po = _po()
    ns, fc, fs = DISTANCES[dist][1], 37, 100
    frames = np.random.default_rng(190).integers(0, 256, (ns, fc * fs)).astype(np.uint8)
    want = po.hca_byte_position_counts(frames, fs, 30)
    d = None
    try:
        d = FarRows(dist, _residue("vga_hca_byte_position_counts_device", "frames"), fc * fs, np.uint8, data=frames)
        counts = np.zeros((30, 256), dtype=np.uint32)
        _ok(_L().vga_hca_byte_position_counts_device(d.ptr, d.pitch, ns, fc, fs, 30, counts.ctypes.data, _stream()))
        assert np.array_equal(counts, want)
        d.clean("frames")
    finally:
        _done(d)


# ====================================================================== the container calls
# (distance, channels, files): rows are files x channels, images are files.  Three images 2^31 apart and four rows 2^31 apart;
# four rows and two images 2^32 apart (16 GiB); two rows 2^33 apart with one image, then two one-channel images 2^33 apart
SHAPES = [("2^31", 1, 3), ("2^31", 2, 2), ("2^32", 2, 2), ("2^33", 2, 1), ("2^33", 1, 2)]
U8 = np.uint8


class _Made(list):
    """the far buffers of a test: freed when the block ends, however it ends"""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _done(*self)

    def far(self, *args, **kw):
        self.append(FarRows(*args, **kw))
        return self[-1]

    def buf(self, dist, far, a, width, dtype, units, data=None, slop=0):
        """far rows, or (one image, a call without a file pitch) a Placed object on a boundary"""
        if far:
            return self.far(dist, a, width, dtype, data=data, units=units, slop=slop)
        return lay.place(data if data is not None else (units, width), lay._round_up(width, 16), 0, dtype)


def _checked(obj, what, out=False):
    if isinstance(obj, FarRows):
        obj.clean(what)
    elif out:
        obj.kept(what, padding=True)
    else:
        obj.unchanged(what)


def _cl():
    import test_gpu_container_layouts as cl
    return cl


@pytest.mark.gpu
@pytest.mark.parametrize("dist,nch,nf", SHAPES)
def test_nwstm_write(dist, nch, nf):
    """BRSTM, BCSTM and BFSTM images of 72-byte interleaves: rows at any byte, images 16 mod 2^k apart (the writer's rule)"""
    cl = _cl()
    for target in cl.NW_TARGETS:
        adpcm, coefs, gain, sc, lc, seek, want, ne = cl._nw_case(target, nch, nf, 126)
        nb, size = adpcm.shape[1], want.shape[1]
        with _Made() as m:
            d_in = m.far(dist, 1, nb, U8, data=adpcm, units=nf * nch)
            d_files = m.buf(dist, nf > 1, 16, size, U8, nf)
            d_seek = lay.place(seek, lay._round_up(2 * ne, 8), 0, np.int16)
            tabs = cl._small_tables((coefs, gain, sc, lc), False)
            p = cl._nw_params(target, 126)
            _ok(_L().vga_nwstm_write_device(C.byref(p), nch, nf, None, d_in.ptr, d_in.pitch, nb, tabs[0].ptr, tabs[1].ptr, tabs[2].ptr,
                                            tabs[3].ptr, d_seek.ptr, d_seek.pitch, ne, d_files.ptr, d_files.pitch, _stream()))
            _torch().cuda.synchronize()
            _eq(d_files.rows(), want, f"images (target {target})")
            _checked(d_files, "images", out=True)
            _checked(d_in, "adpcm")


@pytest.mark.gpu
@pytest.mark.parametrize("dist,nch,nf", SHAPES)
def test_nwstm_read(dist, nch, nf):
    from vgaudio_amd.nwstm import parse
    cl = _cl()
    for target in cl.NW_TARGETS:
        adpcm, _, _, _, _, _, images, _ = cl._nw_case(target, nch, nf, 126)
        nb, size = adpcm.shape[1], images.shape[1]
        info = parse(images[0].tobytes())
        assert (info.adpcm_bytes, info.channel_count) == (nb, nch)
        with _Made() as m:
            d_files = m.buf(dist, nf > 1, 1, size, U8, nf, data=list(images))
            d_rows = m.far(dist, 1, nb, U8, units=nf * nch)
            _ok(_L().vga_nwstm_read_device(C.byref(info), d_files.ptr, d_files.pitch, nf, d_rows.ptr, d_rows.pitch, _stream()))
            _torch().cuda.synchronize()
            _eq(d_rows.rows(), adpcm, f"rows (target {target})")      # (test_gpu_container_layouts.py: the restatement's rows)
            _checked(d_rows, "rows", out=True)
            _checked(d_files, "images")


IDSP_BLOCK, IDSP_TRIM = 0x10, 1


@pytest.mark.gpu
@pytest.mark.parametrize("dist,nch,nf", SHAPES)
def test_idsp_write(dist, nch, nf):
    cl = _cl()
    adpcm, coefs, gain, sc, lc, want = cl._idsp_case(nch, nf, IDSP_BLOCK, IDSP_TRIM)
    nb, size = adpcm.shape[1], want.shape[1]
    with _Made() as m:
        d_in = m.far(dist, 1, nb, U8, data=adpcm, units=nf * nch)
        d_files = m.buf(dist, nf > 1, 16, size, U8, nf)
        tabs = cl._small_tables((coefs, gain, sc, lc), False)
        p = cl._idsp_params(IDSP_BLOCK, IDSP_TRIM)
        _ok(_L().vga_idsp_write_device(C.byref(p), nch, nf, d_in.ptr, d_in.pitch, nb, tabs[0].ptr, tabs[1].ptr, tabs[2].ptr, tabs[3].ptr,
                                       d_files.ptr, d_files.pitch, _stream()))
        _torch().cuda.synchronize()
        _eq(d_files.rows(), want, "images")
        _checked(d_files, "images", out=True)
        _checked(d_in, "adpcm")


@pytest.mark.gpu
@pytest.mark.parametrize("dist,nch,nf", SHAPES)
def test_idsp_read(dist, nch, nf):
    import gc_containers_ref as ref
    from vgaudio_amd.idsp import parse
    cl = _cl()
    adpcm, _, _, _, _, images = cl._idsp_case(nch, nf, IDSP_BLOCK, IDSP_TRIM)
    info = parse(images[0].tobytes())
    ab = info.adpcm_bytes
    want = np.stack([np.frombuffer(r, U8) for f in range(nf) for r in ref.idsp_parse(images[f].tobytes())["audio"]])
    assert want.shape == (nf * nch, ab) and np.array_equal(want, adpcm[:, :ab])
    with _Made() as m:
        d_files = m.buf(dist, nf > 1, 1, images.shape[1], U8, nf, data=list(images))
        d_rows = m.far(dist, 1, ab, U8, units=nf * nch)
        _ok(_L().vga_idsp_read_device(C.byref(info), d_files.ptr, d_files.pitch, nf, d_rows.ptr, d_rows.pitch, _stream()))
        _torch().cuda.synchronize()
        _eq(d_rows.rows(), want, "rows")
        _checked(d_rows, "rows", out=True)
        _checked(d_files, "images")


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["adpcm", "pcm"])
@pytest.mark.parametrize("dist,nch,nf", SHAPES)
def test_hps_write(dist, nch, nf, which):
    """three buffers with a pitch: the images and the ADPCM rows are far together, then the PCM rows behind the block
    headers' histories (three at once pass the 20 GiB of a test at 2^32)"""
    cl = _cl()
    adpcm, pcm, coefs, gain, sc, want = cl._hps_case(nch, nf, False)
    nb, n, size = adpcm.shape[1], pcm.shape[1], want.shape[1]
    with _Made() as m:
        d_in = m.buf(dist, which == "adpcm", 1, nb, U8, nf * nch, data=adpcm)
        d_pcm = m.buf(dist, which == "pcm", 2, n, np.int16, nf * nch, data=pcm)
        d_files = m.buf(dist, which == "adpcm" and nf > 1, 16, size, U8, nf)
        tabs = cl._small_tables((coefs, gain, sc), False)
        p = cl._hps_params(nch, False)
        _ok(_L().vga_hps_write_device(C.byref(p), nch, nf, d_in.ptr, d_in.pitch, nb, tabs[0].ptr, tabs[1].ptr, tabs[2].ptr, d_pcm.ptr,
                                      d_pcm.pitch, n, d_files.ptr, d_files.pitch, _stream()))
        _torch().cuda.synchronize()
        _eq(d_files.rows(), want, "images")
        _checked(d_files, "images", out=True)
        _checked(d_in, "adpcm")
        _checked(d_pcm, "pcm")


@pytest.mark.gpu
@pytest.mark.parametrize("dist,nch,nf", SHAPES)
def test_hps_read(dist, nch, nf):
    from vgaudio_amd.hps import parse
    cl = _cl()
    adpcm, _, _, _, _, images = cl._hps_case(nch, nf, False)
    nb = adpcm.shape[1]
    info, blocks = parse(images[0].tobytes())
    assert info.adpcm_bytes == nb and info.channel_count == nch
    with _Made() as m:
        d_files = m.buf(dist, nf > 1, 1, images.shape[1], U8, nf, data=list(images))
        d_rows = m.far(dist, 1, nb, U8, units=nf * nch)
        _ok(_L().vga_hps_read_device(C.byref(info), blocks, d_files.ptr, d_files.pitch, nf, d_rows.ptr, d_rows.pitch, _stream()))
        _torch().cuda.synchronize()
        _eq(d_rows.rows(), adpcm, "rows")                            # (test_gpu_container_layouts.py: hps_parse's rows)
        _checked(d_rows, "rows", out=True)
        _checked(d_files, "images")


@pytest.mark.gpu
@pytest.mark.parametrize("interleave", [0x40, 6])
@pytest.mark.parametrize("dist,nch,nf", SHAPES)
def test_genh_read(dist, nch, nf, interleave):
    import gc_containers_ref as ref
    from vgaudio_amd.genh import parse
    n = 14 * 300 + 5
    ab = ref.bytes_of(n)
    rng = np.random.default_rng(250 + nch)
    audio = rng.integers(0, 256, (nf, nch, ab)).astype(U8)
    coefs = rng.integers(-32768, 32768, (nch, 16)).tolist()
    images = [np.frombuffer(ref.genh_image(48000, [audio[f, c].tobytes() for c in range(nch)], coefs, interleave, -1, n, 0), U8)
              for f in range(nf)]
    info = parse(images[0].tobytes())
    assert info.adpcm_bytes == ab and info.channel_count == nch
    want = np.stack([np.frombuffer(r, U8) for f in range(nf)
                     for r in ref.deinterleave(images[f][info.audio_data_offset:].tobytes(), ab * nch, interleave, nch)])
    with _Made() as m:
        d_files = m.buf(dist, nf > 1, 1, len(images[0]), U8, nf, data=images)
        d_rows = m.far(dist, 1, ab, U8, units=nf * nch, slop=SLOP)
        _ok(_L().vga_genh_read_device(C.byref(info), d_files.ptr, d_files.pitch, nf, d_rows.ptr, d_rows.pitch, _stream()))
        _torch().cuda.synchronize()
        _eq(d_rows.rows(), want, "rows")
        _checked(d_rows, "rows", out=True)
        _checked(d_files, "images")


def _dsp_images(nch, nf):
    """nf DSP images of nch channels by the oracle's writer, their parsed header and the rows they hold"""
    from vgaudio_amd import _lib
    po = _po()
    n, nb = lay._gc_n(), lay._gc_nb()
    _, coefs, _, _, adpcm, _ = lay._gc().cases()
    args = (48000, n, 0, 0, 0, 14 * 8, 1, 1)
    images = []
    for f in range(nf):
        r = slice(f * nch, (f + 1) * nch)
        rc, img = po.dsp_write(list(adpcm[r]), coefs[r], po.dsp_params(*args))
        assert rc == 0
        images.append(np.asarray(img, dtype=U8))
    info = _lib.DspInfoC()
    _ok(_L().vga_dsp_parse(images[0].ctypes.data_as(_lib.u8p), len(images[0]), C.byref(info)))
    assert info.adpcm_bytes == nb
    return images, info, adpcm[:nf * nch]


@pytest.mark.gpu
@pytest.mark.parametrize("dist,nch,nf", SHAPES)
def test_dsp_read(dist, nch, nf):
    images, info, want = _dsp_images(nch, nf)
    with _Made() as m:
        d_files = m.buf(dist, nf > 1, 1, len(images[0]), U8, nf, data=images)
        d_rows = m.far(dist, 1, want.shape[1], U8, units=nf * nch)
        _ok(_L().vga_dsp_read_device(C.byref(info), d_files.ptr, d_files.pitch, nf, d_rows.ptr, d_rows.pitch, _stream()))
        _torch().cuda.synchronize()
        _eq(d_rows.rows(), want, "rows")
        _checked(d_rows, "rows", out=True)
        _checked(d_files, "images")


@pytest.mark.gpu
@pytest.mark.parametrize("dist", DIST)
def test_dsp_write(dist):
    """one image a call: its channels are the far rows"""
    from vgaudio_amd import _lib
    po = _po()
    nch = DISTANCES[dist][1]
    n, nb = lay._gc_n(), lay._gc_nb()
    _, coefs, _, _, adpcm, _ = lay._gc().cases()
    args = (48000, n, 1, 140, 8000, 14 * 64, 1, 0)
    rng = np.random.default_rng(240 + nch)
    gain = rng.integers(-32768, 32768, nch).astype(np.int16)
    sc, lc = rng.integers(-32768, 32768, (nch, 3)).astype(np.int16), rng.integers(-32768, 32768, (nch, 3)).astype(np.int16)
    rc, want = po.dsp_write(list(adpcm[:nch]), coefs[:nch], po.dsp_params(*args), gain=gain, start_context=sc, loop_context=lc)
    assert rc == 0
    p = _lib.DspParamsC(*args)
    with _Made() as m:
        d_in = m.far(dist, 8, nb, U8, data=adpcm[:nch])                 # the codec's rows: multiples of 8
        d_file = lay.place((1, len(want)), len(want), 0, U8)
        d_coefs, d_gain, d_sc, d_lc = (lay._up(v) for v in (coefs[:nch], gain, sc, lc))
        _ok(_L().vga_dsp_write_device(d_in.ptr, d_in.pitch, nb, d_coefs.data_ptr(), d_gain.data_ptr(), d_sc.data_ptr(), d_lc.data_ptr(), nch,
                                      C.byref(p), d_file.ptr, _stream()))
        _torch().cuda.synchronize()
        _eq(d_file.rows()[0], np.asarray(want, dtype=U8), "image")
        d_file.kept("image", padding=True)
        d_in.clean("adpcm")


@pytest.mark.gpu
@pytest.mark.parametrize("dist", DIST)
def test_adx_write(dist):
    from vgaudio_amd import _lib
    cl = _cl()
    nch = DISTANCES[dist][1]
    for version, fs in ((4, 18), (4, 34)):
        audio, hist, want = cl._adx_case(version, nch, fs, 0)
        n, nb, G = cl._adx_geometry(version, nch, fs, 0)
        p = _lib.AdxFileParamsC(cl.ADX_RATE, n, 0, 0, 0, 0, fs, version, 3, 500, 0, 1)
        with _Made() as m:
            d_in = m.far(dist, 1, nb, U8, data=audio)
            d_hist = lay.small(hist, 0, np.int16)
            d_file = lay.place((1, G["file_size"]), G["file_size"], 0, U8)
            _ok(_L().vga_adx_write_device(d_in.ptr, d_in.pitch, nb, d_hist.ptr, nch, C.byref(p), d_file.ptr, _stream()))
            _torch().cuda.synchronize()
            _eq(d_file.rows()[0], want, "image")
            d_file.kept("image", padding=True)
            d_in.clean("audio")


@pytest.mark.gpu
@pytest.mark.parametrize("general", [0, 1])
@pytest.mark.parametrize("dist,nch,nf", SHAPES)
def test_adx_read(dist, nch, nf, general):
    """images by oracle/pyref's writer; both forms of the read (the span kernel and the general one)"""
    from oracle.pyref import containers as rcont
    from vgaudio_amd import _lib
    cl = _cl()
    L = _L()
    n, nb, G = cl._adx_geometry(4, nch, 18, 0)
    rng = np.random.default_rng(260 + nch)
    audio = rng.integers(0, 256, (nf * nch, nb)).astype(U8)
    hist = rng.integers(-32768, 32768, nch).astype(np.int16)
    images = [np.frombuffer(rcont.adx_write([a.tobytes() for a in audio[f * nch:(f + 1) * nch]], hist.tolist(), cl.ADX_RATE, n,
                                            frame_size=18, version=4), U8) for f in range(nf)]
    info = _lib.AdxFileInfoC()
    _ok(L.vga_adx_parse(images[0].ctypes.data_as(_lib.u8p), len(images[0]), C.byref(info)))
    assert info.audio_bytes == nb
    with _Made() as m:
        d_files = m.buf(dist, nf > 1, 1, len(images[0]), U8, nf, data=images)
        d_rows = m.far(dist, 1, nb, U8, units=nf * nch)
        old = L.vga_testing_adx_read_general_this_thread(general)
        try:
            _ok(L.vga_adx_read_device(C.byref(info), d_files.ptr, d_files.pitch, nf, d_rows.ptr, d_rows.pitch, _stream()))
        finally:
            L.vga_testing_adx_read_general_this_thread(old)
        _torch().cuda.synchronize()
        _eq(d_rows.rows(), audio, "rows")
        _checked(d_rows, "rows", out=True)
        _checked(d_files, "images")


@pytest.mark.gpu
@pytest.mark.parametrize("dist", DIST)
def test_hca_write(dist):
    cl = _cl()
    ns = DISTANCES[dist][1]
    info, frames, want = cl._hca_case(None)
    audio, size = frames.shape[1], want.shape[1]
    with _Made() as m:
        d_in = m.far(dist, 1, audio, U8, data=frames[:ns])
        d_files = m.far(dist, 1, size, U8)
        _ok(_L().vga_hca_write_device(C.byref(info), d_in.ptr, d_in.pitch, ns, None, 1.0, 0, 0, d_files.ptr, d_files.pitch, _stream()))
        _torch().cuda.synchronize()
        _eq(d_files.rows(), want[:ns], "images")
        d_files.clean("images")
        d_in.clean("frames")


@pytest.mark.gpu
@pytest.mark.parametrize("dist", DIST)
def test_hca_read(dist):
    """the images of test_hca_write (random frames: every CRC is wrong, and counted); frames and 8 zero bytes a row"""
    import container_readers_ref as rref
    from vgaudio_amd import _lib
    cl = _cl()
    torch = _torch()
    nf = DISTANCES[dist][1]
    H, frames, images = cl._hca_case(None)
    audio = frames.shape[1]
    info = _lib.HcaFileInfoC()
    img0 = np.ascontiguousarray(images[0])
    _ok(_L().vga_hca_parse(img0.ctypes.data_as(_lib.u8p), len(img0), C.byref(info)))
    assert info.hca.frame_count * info.hca.frame_size == audio
    want_bad = [rref.bad_crc_frames(frames[f].reshape(H.frame_count, H.frame_size)) for f in range(nf)]
    assert min(want_bad) > 0
    with _Made() as m:
        d_files = m.far(dist, 1, images.shape[1], U8, data=list(images[:nf]))
        d_rows = m.far(dist, 4, audio + 8, U8, slop=4)               # rows vga_hca_decode_device takes: multiples of 4 (and the
                                                                     # read may round a row's end up to one)
        bad = torch.full((nf,), -1, dtype=torch.int32, device="cuda")
        _ok(_L().vga_hca_read_device(C.byref(info), d_files.ptr, d_files.pitch, nf, d_rows.ptr, d_rows.pitch, bad.data_ptr(), _stream()))
        torch.cuda.synchronize()
        _eq(d_rows.rows(), np.concatenate([frames[:nf], np.zeros((nf, 8), U8)], axis=1), "frames and their slack")
        assert bad.cpu().tolist() == want_bad
        d_rows.clean("frames")
        d_files.clean("images")


@pytest.mark.gpu
@pytest.mark.parametrize("dist", DIST)
def test_synth_pcm16(dist):
    from vgaudio_amd import synth
    nch, n, first = DISTANCES[dist][1], 1000 + 3, 7
    want = synth.generate(nch, n, first_channel=first)
    params = np.array([synth.channel_params(first + c) for c in range(nch)], dtype=np.uint32)
    with _Made() as m:
        d_params = lay.small(params, 0, np.uint32)
        d_pcm = m.far(dist, 2, n, np.int16)
        _ok(_L().vga_synth_pcm16_device(d_pcm.ptr, d_pcm.pitch, nch, n, first, d_params.ptr, _stream()))
        _torch().cuda.synchronize()
        _eq(d_pcm.rows(), np.asarray(want, dtype=np.int16), "pcm")
        d_pcm.clean("pcm")


@pytest.mark.gpu
@pytest.mark.parametrize("signed", [0, 1])
@pytest.mark.parametrize("dist", DIST)
def test_pcm8_encode(dist, signed):
    rows, n = DISTANCES[dist][1], 1000 + 3
    pcm = np.random.default_rng(270 + signed).integers(-32768, 32768, (rows, n)).astype(np.int16)
    pcm[0, :4] = (-32768, 32767, -1, 0)
    s = pcm.astype(np.int32)
    want = ((s >> 8) if signed else ((s + 0x8000) >> 8)).astype(U8)
    with _Made() as m:
        d_in = m.far(dist, 2, n, np.int16, data=pcm)
        d_out = m.far(dist, 1, n, U8)
        _ok(_L().vga_pcm8_encode_device(d_in.ptr, d_in.pitch, n, rows, signed, d_out.ptr, d_out.pitch, _stream()))
        _torch().cuda.synchronize()
        _eq(d_out.rows(), want, "bytes")
        d_out.clean("bytes")
        d_in.clean("pcm")


@pytest.mark.gpu
@pytest.mark.parametrize("signed", [0, 1])
@pytest.mark.parametrize("dist", DIST)
def test_pcm8_decode(dist, signed):
    rows, n = DISTANCES[dist][1], 1000 + 3
    data = np.random.default_rng(272 + signed).integers(0, 256, (rows, n)).astype(U8)
    data[0, :4] = (0, 0x7f, 0x80, 0xff)
    b = data.astype(np.int32)
    want = (((b ^ 0x80) - 0x80) * 256 if signed else (b - 0x80) * 256).astype(np.int16)
    with _Made() as m:
        d_in = m.far(dist, 1, n, U8, data=data)
        d_out = m.far(dist, 2, n, np.int16)
        _ok(_L().vga_pcm8_decode_device(d_in.ptr, d_in.pitch, n, rows, signed, d_out.ptr, d_out.pitch, _stream()))
        _torch().cuda.synchronize()
        _eq(d_out.rows(), want, "pcm")
        d_out.clean("pcm")
        d_in.clean("bytes")


@pytest.mark.gpu
@pytest.mark.parametrize("dist", DIST)
def test_wave_pcm16(dist):
    """vga_wave_write_pcm16_device from far rows against the oracle's image, then vga_wave_deinterleave_pcm16_device of that
    image's data chunk into far rows"""
    from vgaudio_amd import _lib
    po = _po()
    L = _L()
    nch, n = DISTANCES[dist][1], 10007
    pcm = np.random.default_rng(280).integers(-32768, 32768, (nch, n)).astype(np.int16)
    rc, want = po.wave_write(list(pcm), 48000)
    assert rc == 0
    want = np.frombuffer(want.tobytes(), U8)
    p = _lib.WaveParamsC(48000, n, 0, 0, 0)
    assert L.vga_wave_file_size(C.byref(p), nch) == len(want)
    with _Made() as m:
        d_pcm = m.far(dist, 2, n, np.int16, data=pcm)
        d_file = lay.place((1, len(want)), len(want), 0, U8)
        _ok(L.vga_wave_write_pcm16_device(d_pcm.ptr, d_pcm.pitch, nch, C.byref(p), d_file.ptr, _stream()))
        _torch().cuda.synchronize()
        _eq(d_file.rows()[0], want, "image")
        d_file.kept("image", padding=True)
        d_pcm.clean("pcm")
    data = want[len(want) - 2 * nch * n:]
    with _Made() as m:
        d_data = lay.place([data], len(data), 0, U8)
        d_rows = m.far(dist, 2, n, np.int16)
        _ok(L.vga_wave_deinterleave_pcm16_device(d_data.ptr, n, nch, d_rows.ptr, d_rows.pitch, _stream()))
        _torch().cuda.synchronize()
        _eq(d_rows.rows(), pcm, "rows")
        d_rows.clean("rows")
        d_data.unchanged("data")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("dist", DIST)
def test_wave_pcm8(dist, kind):
    """vga_wave_write_pcm8_device and vga_wave_deinterleave_pcm8_device, int16 rows and byte rows"""
    from vgaudio_amd import _lib
    cl = _cl()
    L = _L()
    nch = DISTANCES[dist][1]
    rows, back, want = cl._wave_case(nch, kind)
    es = rows.dtype.itemsize
    p = _lib.WaveParamsC(cl.WAVE_RATE, cl.WAVE_N, 0, 0, 0)
    with _Made() as m:
        d_in = m.far(dist, es, cl.WAVE_N, rows.dtype, data=rows)
        d_file = lay.place((1, len(want)), len(want), 0, U8)
        _ok(L.vga_wave_write_pcm8_device(d_in.ptr, kind, d_in.pitch, nch, C.byref(p), d_file.ptr, _stream()))
        _torch().cuda.synchronize()
        _eq(d_file.rows()[0], want, "image")
        d_file.kept("image", padding=True)
        d_in.clean("rows")
    data = want[len(want) - nch * cl.WAVE_N:]
    with _Made() as m:
        d_data = lay.place([data], len(data), 0, U8)
        d_rows = m.far(dist, es, cl.WAVE_N, rows.dtype)
        _ok(L.vga_wave_deinterleave_pcm8_device(d_data.ptr, cl.WAVE_N, nch, d_rows.ptr, kind, d_rows.pitch, _stream()))
        _torch().cuda.synchronize()
        _eq(d_rows.rows(), back, "rows")
        d_rows.clean("rows")
        d_data.unchanged("data")


def _nw_pcm_case(k, nch, nf, spi=255):
    """test_gpu_container_layouts.py's _pcm_case for nf images of nch channels"""
    import nwstm_pcm_ref as ref
    cl = _cl()
    codec, kind, big = cl.PCM_KINDS[k]
    rng = np.random.default_rng(290 + 10 * k + nch + nf)
    shape = (nf * nch, cl.PCM_N)
    rows = (rng.integers(-32768, 32768, shape).astype(np.int16) if kind == cl.S16 else rng.integers(0, 256, shape).astype(U8))
    eight = codec == cl.PCM8 and kind == cl.S16
    stored = ref.encode_signed(rows) if eight else rows
    back = ref.decode_signed(stored) if eight else rows
    images = np.stack([np.frombuffer(ref.build_image(ref.FSTM, codec, cl.PCM_RATE, list(stored[f * nch:(f + 1) * nch]), spi=spi, big=big), U8)
                       for f in range(nf)])
    p = cl._pcm_params(k, spi)
    return codec, kind, rows, back, images, p


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("dist,nch,nf", SHAPES)
def test_nwstm_pcm_write(dist, nch, nf, k):
    """PCM16 big- and little-endian, PCM8 from int16 rows and from byte rows; 255-sample interleaves"""
    codec, kind, rows, _, want, p = _nw_pcm_case(k, nch, nf)
    with _Made() as m:
        d_in = m.far(dist, rows.dtype.itemsize, rows.shape[1], rows.dtype, data=rows, units=nf * nch)
        d_files = m.buf(dist, nf > 1, 16, want.shape[1], U8, nf)
        _ok(_L().vga_nwstm_pcm_write_device(C.byref(p), codec, nch, nf, None, d_in.ptr, kind, d_in.pitch, d_files.ptr, d_files.pitch,
                                            _stream()))
        _torch().cuda.synchronize()
        _eq(d_files.rows(), want, "images")
        _checked(d_files, "images", out=True)
        _checked(d_in, "rows")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("dist,nch,nf", SHAPES)
def test_nwstm_pcm_read(dist, nch, nf, k):
    from vgaudio_amd.nwstm import parse_pcm
    codec, kind, rows, want, images, _ = _nw_pcm_case(k, nch, nf)
    info = parse_pcm(images[0].tobytes())
    assert (info.sample_count, info.channel_count) == (rows.shape[1], nch)
    with _Made() as m:
        d_files = m.buf(dist, nf > 1, 1, images.shape[1], U8, nf, data=list(images))
        d_rows = m.far(dist, rows.dtype.itemsize, rows.shape[1], rows.dtype, units=nf * nch)
        _ok(_L().vga_nwstm_pcm_read_device(C.byref(info), d_files.ptr, d_files.pitch, nf, d_rows.ptr, kind, d_rows.pitch, _stream()))
        _torch().cuda.synchronize()
        _eq(d_rows.rows(), want, "rows")
        _checked(d_rows, "rows", out=True)
        _checked(d_files, "images")


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["adpcm", "pcm+seek"])
@pytest.mark.parametrize("dist", DIST)
def test_gc_build_channels(dist, which):
    """four buffers with a pitch: ADPCM in and out far together, then the PCM and the seek table"""
    from vgaudio_amd import _lib
    torch = _torch()
    L = _L()
    po = _po()
    n, loop, alignment, spe, _, coefs, adpcm, want = lay._build_channels_case()
    nch = DISTANCES[dist][1]
    ly = want[0][1]
    ns, ne = ly.sample_count_aligned, ly.seek_table_entries
    na, nb = po.gc_sample_count_to_byte_count(ns), adpcm.shape[1]
    p = _lib.GcChannelParamsC(n, 1, loop[0], loop[1], alignment, spe)
    far_a, far_p = which == "adpcm", which != "adpcm"
    with _Made() as m:
        d_in = m.buf(dist, far_a, 8, nb, U8, nch, data=adpcm[:nch])
        a_out = m.buf(dist, far_a, 8, na, U8, nch, slop=SLOP)
        p_out = m.buf(dist, far_p, 4, ns, np.int16, nch, slop=SLOP)
        s_out = m.buf(dist, far_p, 2, 2 * ne, np.int16, nch, slop=SLOP)
        c_out = lay.place((1, nch * 3), nch * 3, 0, np.int16)
        d_coefs = lay._up(coefs[:nch])
        wsb = L.vga_gcadpcm_build_channels_workspace_bytes(nch, C.byref(p))
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
        _ok(L.vga_gcadpcm_build_channels_device(d_in.ptr, d_in.pitch, d_coefs.data_ptr(), nch, C.byref(p), a_out.ptr, a_out.pitch, p_out.ptr,
                                                p_out.pitch, s_out.ptr, s_out.pitch, c_out.ptr, ws.data_ptr(), wsb, _stream()))
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
            if isinstance(q, FarRows):
                q.clean(what)
            else:
                q.kept(what)
        _checked(d_in, "adpcm in")


# ====================================================================== file sets at the caller's offsets
# Six small files of the *_files_cases.py a set: at 0, ending just below 2^31, across 2^32 (the carry falls inside a row or
# an image), just behind it, across 2^33 and behind that.  The buffer the set addresses begins LEAD bytes into its allocation,
# so that an offset between 2^31 and 2^32 read as a negative number still lands inside; one cut to 32 bits does anyway.
LEAD = 1 << 31
JUNK = 0xEE
EXTRA = 64


def far_spots(file_rows, residue, align=16):
    """file_rows: per file the byte counts of its rows (or its one image) -> one offset per row, each `residue` past a
    multiple of `align`, the rows of a file one behind the other"""
    assert len(file_rows) == 6 and all(rows and min(rows) > 0 for rows in file_rows)
    up = lay._round_up

    def within(rows):                                            # offsets of the rows from the file's first, and its length
        at, out = 0, []
        for r in rows:
            out.append(at)
            at += up(r + residue, align)
        return out, at

    def across(rows, mark):                                      # the middle of the file's longest row on the mark
        rel, _ = within(rows)
        k = int(np.argmax(rows))
        assert rows[k] >= 4 * align
        return (mark - rel[k] - rows[k] // 2) // align * align

    rel = [within(rows) for rows in file_rows]
    start = [0, ((1 << 31) - rel[1][1] - align) // align * align, across(file_rows[2], 1 << 32)]
    start.append(up(start[2] + rel[2][1], align) + align)
    start.append(across(file_rows[4], 1 << 33))
    start.append(up(start[4] + rel[4][1], align) + align)
    offs = [s + residue + o for s, (o_list, _) in zip(start, rel) for o in o_list]
    return offs


def test_far_spots_lie_where_the_issue_puts_them():
    """(CPU) for the row sizes of every set below: file 1 ends under 2^31, a row of file 2 holds byte 2^32 and one of file 4
    byte 2^33, files 3 and 5 begin within a page behind them, nothing overlaps"""
    for rows, residue in (([[36, 36], [400], [126, 126, 126], [1000] * 4, [1692] * 8, [8082, 8082]], 4), ([[98], [700], [64], [5000], [90], [2000]], 3),
                          ([[45], [16368], [16027], [20460], [4781], [682]], 0)):
        offs = far_spots(rows, residue)
        flat = [r for f in rows for r in f]
        spans = sorted(zip(offs, flat))
        assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])) and all(o % 16 == residue for o in offs)
        first = np.cumsum([0] + [len(f) for f in rows])
        ends = [max(offs[c] + flat[c] for c in range(first[k], first[k + 1])) for k in range(6)]
        assert offs[0] == residue and (1 << 31) - 128 <= ends[1] < 1 << 31
        for k, mark in ((2, 1 << 32), (4, 1 << 33)):
            assert any(offs[c] < mark < offs[c] + flat[c] for c in range(first[k], first[k + 1]))
            assert mark < offs[first[k + 1]] < mark + 32768 and ends[k] <= offs[first[k + 1]]


def _far_source(total, pieces):
    """a FarBuffer that holds `total` bytes LEAD bytes in, with pieces (offset, array) put there: (buffer, windows)"""
    extent = lay._round_up(LEAD + total + TAIL, 256)
    fm.need(extent)
    buf = fm.FarBuffer(extent)
    return buf, [buf.put(LEAD + int(o), a) for o, a in pieces]


def _unchanged(buf, windows, pieces, what):
    for (o, n), (_, a) in zip(windows, pieces):
        assert np.array_equal(buf.get(o, n), np.ascontiguousarray(a).view(U8).reshape(-1)), (what, "an input changed", o - LEAD)
    first = buf.untouched(windows)
    assert first is None, (what, buf.changed, "bytes around the far input changed, the first at", first - LEAD)


def _near_out(nbytes):
    return _torch().full((nbytes + 2 * EXTRA,), JUNK, dtype=_torch().uint8, device="cuda")


def _near_is(out, wanted, what):
    """out: a _near_out buffer; wanted: (offset, array) -- those bytes and nothing else were written"""
    got = out.cpu().numpy().copy()
    for k, (at, want) in enumerate(wanted):
        mine = got[EXTRA + int(at):EXTRA + int(at) + len(want)]
        assert np.array_equal(mine, want), (what, "piece", k, "first bad byte", int(np.flatnonzero(mine != want)[0]))
        mine[:] = JUNK
    assert np.all(got == JUNK), (what, "bytes outside were written", np.flatnonzero(got != JUNK)[:8] - EXTRA)


ADX_SET = [1, 6, 14, 16, 17, 18]          # of adx_files_cases.CASES: 18-, 19- and 36-byte frames, 2 to 8 channels, loops, one span file


def _adx_pick(per_file, per_row, files):
    first = np.cumsum([0] + [f.channels for f in files])
    return [per_file[k] for k in ADX_SET], [[per_row[c] for c in range(first[k], first[k + 1])] for k in ADX_SET]


@pytest.mark.gpu
@pytest.mark.parametrize("residue", [0, 4])
def test_adx_files_write_from_far_rows(residue):
    """vga_adx_files_create with audio_offsets, vga_adx_write_device_v: rows at multiples of 16 (the span form where a file
    qualifies) and 4 past them (the general form throughout); the images are the oracle's AdxWriter's"""
    import test_gpu_adx_files as ta
    from vgaudio_amd.adx import AdxFileSet
    files, _, rows, hist, want = ta.reference("packed")
    _, hist = _adx_pick(want, list(hist), files)
    want, rows = _adx_pick(want, rows, files)
    files = [files[k] for k in ADX_SET]
    flat = [r for f in rows for r in f]
    offs = far_spots([[len(r) for r in f] for f in rows], residue)
    s = AdxFileSet(files, offs)
    buf = None
    try:
        assert list(s.audio_offsets) == offs and s.totals.audio_bytes > 1 << 33
        span, general = s.stats()[:2]
        assert (span > 0) == (residue == 0) and general > 0
        pieces = list(zip(offs, flat))
        buf, windows = _far_source(s.totals.audio_bytes, pieces)
        images = _near_out(s.totals.image_bytes)
        d_hist = lay._up(np.array([h for f in hist for h in f], np.int16))
        _ok(_L().vga_adx_write_device_v(s._h, buf.ptr + LEAD, d_hist.data_ptr(), images.data_ptr() + EXTRA, _stream()))
        _torch().cuda.synchronize()
        _near_is(images, list(zip(s.image_offsets, want)), "images")
        _unchanged(buf, windows, pieces, "rows")
    finally:
        s.close()
        fm.release(buf)


@pytest.mark.gpu
@pytest.mark.parametrize("residue", [0, 3])
def test_adx_files_read_from_far_images(residue):
    """vga_adx_files_create_from_infos with image_offsets, vga_adx_read_device_v: the rows and start histories are the
    oracle's AdxReader's"""
    import test_gpu_adx_files as ta
    from vgaudio_amd.adx import AdxFileSet
    torch = _torch()
    files, want, infos, audio = ta.read_reference()
    want, infos, audio = ([x[k] for k in ADX_SET] for x in (want, infos, audio))
    sizes = [i.audio_offset + i.audio_bytes * i.channel_count for i in infos]
    offs = far_spots([[n] for n in sizes], residue)
    s = AdxFileSet.from_infos(infos, offs)
    buf = None
    try:
        assert list(s.image_offsets) == offs and s.totals.image_bytes > 1 << 33
        pieces = [(o, w[:n]) for o, w, n in zip(offs, want, sizes)]
        buf, windows = _far_source(s.totals.image_bytes, pieces)
        rows = _near_out(s.totals.audio_bytes)
        hist = torch.full((s.channels + 8,), 0x7777, dtype=torch.int16, device="cuda")
        _ok(_L().vga_adx_read_device_v(s._h, buf.ptr + LEAD, rows.data_ptr() + EXTRA, hist.data_ptr(), _stream()))
        torch.cuda.synchronize()
        wanted, c = [], 0
        for f, info in enumerate(infos):
            for ch in range(info.channel_count):
                wanted.append((s.audio_offsets[c], np.asarray(audio[f][ch][:info.audio_bytes], dtype=U8)))
                c += 1
        _near_is(rows, wanted, "rows")
        h = hist.cpu().numpy()
        assert list(h[:s.channels]) == [int(i.history[c][0]) for i in infos for c in range(i.channel_count)] and np.all(h[s.channels:] == 0x7777)
        _unchanged(buf, windows, pieces, "images")
    finally:
        s.close()
        fm.release(buf)


HCA_SET = [3, 4, 5, 10, 12, 9]            # of hca_files_cases.CASES: keyed and not, loops, damaged frames in files 5 and 10


@pytest.mark.gpu
def test_hca_files_write_from_far_frames():
    """vga_hca_files_create with frame_offsets, vga_hca_write_device_v: the images are the oracle's CryptFrame and HcaWriter's"""
    import test_gpu_hca_files as th
    from vgaudio_amd.hca import HcaFileSet
    r = th.reference()
    files, frames, want = ([r[key][k] for k in HCA_SET] for key in ("files", "frames", "want"))
    offs = far_spots([[len(fr)] for fr in frames], 4)
    s = HcaFileSet(files, offs, r["enc"])
    buf = None
    try:
        assert list(s.frame_offsets) == offs and s.totals.frame_bytes > 1 << 33
        pieces = list(zip(offs, frames))
        buf, windows = _far_source(s.totals.frame_bytes, pieces)
        images = _near_out(s.totals.image_bytes)
        _ok(_L().vga_hca_write_device_v(s._h, buf.ptr + LEAD, images.data_ptr() + EXTRA, _stream()))
        _torch().cuda.synchronize()
        _near_is(images, list(zip(s.image_offsets, want)), "images")
        _unchanged(buf, windows, pieces, "frames")
    finally:
        s.close()
        fm.release(buf)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["images", "frames"])
def test_hca_files_read_far(which):
    """vga_hca_files_create_from_infos and vga_hca_read_device_v, the images at far image_offsets (any byte), then the
    frames delivered to far frame_offsets: the oracle's frames, its bad-CRC counts, zeros up to a multiple of 4"""
    import hca_files_cases as hc
    import test_gpu_hca_files as th
    from vgaudio_amd.hca import HcaFileSet
    torch = _torch()
    r = th.reference()
    stored, infos, back, bad = ([r[key][k] for k in HCA_SET] for key in ("stored", "infos", "back", "bad"))
    assert sum(bad) >= 7
    image_offs = far_spots([[len(s)] for s in stored], 3) if which == "images" else None
    frame_offs = far_spots([[len(b)] for b in back], 4) if which == "frames" else None
    s = HcaFileSet.from_infos(infos, image_offs, [hc.CASES[k][8] for k in HCA_SET], r["dec"], frame_offs)
    buf = None
    try:
        assert max(s.totals.image_bytes, s.totals.frame_bytes) > 1 << 33
        counts = torch.zeros(s.files, dtype=torch.int32, device="cuda")
        padded = [np.concatenate([b, np.zeros(-len(b) % 4, U8)]) for b in back]
        if which == "images":
            pieces = list(zip(image_offs, stored))
            buf, windows = _far_source(s.totals.image_bytes, pieces)
            frames = _near_out(s.totals.frame_bytes)
            _ok(_L().vga_hca_read_device_v(s._h, buf.ptr + LEAD, frames.data_ptr() + EXTRA, counts.data_ptr(), _stream()))
            torch.cuda.synchronize()
            _near_is(frames, list(zip(s.frame_offsets, padded)), "frames")
            _unchanged(buf, windows, pieces, "images")
        else:
            images = np.full(s.totals.image_bytes, JUNK, U8)
            for at, image in zip(s.image_offsets, stored):
                images[at:at + len(image)] = image
            d_images = lay._up(images)
            buf, windows = _far_source(s.totals.frame_bytes, [])
            _ok(_L().vga_hca_read_device_v(s._h, d_images.data_ptr(), buf.ptr + LEAD, counts.data_ptr(), _stream()))
            torch.cuda.synchronize()
            for k, (o, want) in enumerate(zip(frame_offs, padded)):
                _eq(buf.get(LEAD + o, len(want)), want, f"frames of file {k}")
            first = buf.untouched([(LEAD + o, len(p)) for o, p in zip(frame_offs, padded)])
            assert first is None, (buf.changed, "bytes outside the streams were written, the first at", first - LEAD)
            assert np.array_equal(d_images.cpu().numpy(), images)
        assert counts.cpu().tolist() == bad
    finally:
        s.close()
        fm.release(buf)


GC_SET = [1, 3, 5, 6, 4, 9]               # of gc_files_cases.FILES: 2, 3 and 6 channels, loops, a file without a seek table
SENTINEL = 0x5BCD


def _i16_out(n):
    return _torch().full((n + EXTRA,), SENTINEL, dtype=_torch().int16, device="cuda")


def _i16_is(t, want, what):
    got = t.cpu().numpy()
    want = np.asarray(want, np.int16).reshape(-1)
    assert np.array_equal(got[:want.size], want) and np.all(got[want.size:] == SENTINEL), what


@pytest.mark.gpu
def test_dsp_files_read_from_far_images():
    """vga_gc_files_create_from_dsp with image_offsets (multiples of 8), vga_dsp_read_device_v: rows, coefficients, gains and
    contexts are the oracle's dsp_read's, as in test_gpu_gc_files.py (8-byte interleave blocks, trimmed files)"""
    import test_gpu_gc_files as tg
    images = [tg.oracle_images("blocks8", 1)[k] for k in GC_SET]
    offs = far_spots([[img.size] for img in images], 8)
    r = tg.ReadSet(images, offs)
    buf = None
    try:
        s, nch = r.s, r.s.channels
        assert list(s.image_offsets) == offs and r.t.image_bytes > 1 << 33
        pieces = list(zip(offs, images))
        buf, windows = _far_source(r.t.image_bytes, pieces)
        rows = _near_out(r.t.adpcm_bytes)
        coefs, gain, start, loop = _i16_out(nch * 16), _i16_out(nch), _i16_out(nch * 3), _i16_out(nch * 3)
        _ok(_L().vga_dsp_read_device_v(s._h, buf.ptr + LEAD, rows.data_ptr() + EXTRA, coefs.data_ptr(), gain.data_ptr(), start.data_ptr(),
                                       loop.data_ptr(), _stream()))
        _torch().cuda.synchronize()
        _near_is(rows, [(at, np.asarray(w["adpcm"], dtype=U8)) for w, at in zip(r.want, r.ao)], "rows")
        for t, key in ((coefs, "coefs"), (gain, "gain"), (start, "start"), (loop, "loop")):
            _i16_is(t, np.concatenate([np.atleast_1d(w[key]).reshape(-1) for w in r.want]), key)
        _unchanged(buf, windows, pieces, "images")
    finally:
        r.close()
        fm.release(buf)


# ====================================================================== packed objects, with ballast in front of the probes
# An object that packs its own buffers reaches a far offset only with bulk in front of it.  The bulk is one channel of
# UNIT samples replicated: unit 0, at the start of every buffer, is held to the oracle, every other unit's output must equal
# unit 0's on the device (torch.equal on slices), the units that straddle 2^31 and 2^32 included.  Behind the first ballast
# unit that ends past 2^31 and 2^32 bytes of EACH packed buffer of the object comes a group of probes: short channels with
# lengths of test_gpu_ragged.py's AWKWARD, each held to the oracle.  Nothing reaches 2^33 here (README).
UNIT = (1 << 22) - 14 * 37 - 3            # ballast samples: no multiple of 14 or 8, so rows end inside a frame and a vector
PROBES = (1, 13, 14, 29, 8 * 14 + 1, 3072 * 14 + 5)
MARKS = (1 << 31, 1 << 32)


def _ballast_plan(unit_bytes):
    """unit_bytes: the room one ballast unit takes in each packed buffer.  -> the lengths of all channels and, per probe
    group, the index of its first channel: groups after the first ballast unit that ends past each mark of each buffer, one
    more ballast unit behind the last group"""
    cuts = sorted({-(-m // b) for b in unit_bytes for m in MARKS})       # ballast units in front of each group
    counts, groups, done = [], [], 0
    for k in cuts:
        counts += [UNIT] * (k - done)
        groups.append(len(counts))
        counts += list(PROBES)
        done = k
    return counts + [UNIT], groups


def _replicate(flat, unit0, offsets, counts):
    """unit0 (a device tensor) to every ballast row of the flat packed tensor"""
    for o, n in zip(offsets, counts):
        if n == UNIT:
            flat[int(o):int(o) + UNIT] = unit0


def _ballast_equal(flat, offsets, counts, width, what):
    """every ballast row of `flat` (width elements from its offset) equals the first one, on the device"""
    torch = _torch()
    rows = [int(o) for o, n in zip(offsets, counts) if n == UNIT]
    first = flat[rows[0]:rows[0] + width]
    same = torch.stack([(flat[o:o + width] == first).all() for o in rows[1:]])
    bad = torch.nonzero(~same).reshape(-1).cpu().tolist()
    assert not bad, (what, "ballast units that differ from unit 0", [(k + 1, rows[k + 1]) for k in bad[:8]], len(bad))


@pytest.mark.gpu
def test_gc_packed_chain():
    """vga_gcadpcm_coefs_device_v, vga_gcadpcm_encode_device_v and vga_gcadpcm_decode_device_v on one batch whose packed PCM
    passes 2^32 BYTES at its 512th ballast unit and whose packed ADPCM passes 2^31 and 2^32 bytes far behind that: four
    groups of probes.  Rows are compared over the 16 bytes the layout rounds them to; between the slots nothing may change."""
    from vgaudio_amd.device import GcRaggedBatch
    torch = _torch()
    L = _L()
    po = _po()
    nb_unit = int(L.vga_gcadpcm_sample_count_to_byte_count(UNIT))
    counts, groups = _ballast_plan((lay._round_up(UNIT, 8) * 2, lay._round_up(nb_unit, 16)))
    r = GcRaggedBatch(counts, "cuda")
    pcm = adpcm = dec = None
    try:
        nch = r.nch
        po_, ao = r.pcm_offsets, r.adpcm_offsets
        firsts = [int(po_[g]) * 2 for g in groups] + [int(ao[g]) for g in groups]
        for m in MARKS:                                          # a group begins within a ballast unit behind each mark of each buffer
            room = 1 << 20                                       # (the probes of the groups in front)
            assert any(m <= f < m + (1 << 23) + room for f in firsts[:len(groups)]) and any(m <= f < m + nb_unit + room for f in firsts[len(groups):])
        need = r.pcm_samples * 4 + r.adpcm_bytes + r.workspace_bytes
        assert need < 46 * GIB, need
        fm.need(need)
        # inputs: the ballast channel and the probes' channels, junk in the rounding
        host = [po.synth_generate(1, n, first_channel=900 + c)[0] for c, n in enumerate(PROBES)]
        unit = po.synth_generate(1, UNIT, first_channel=899)[0]
        pcm = fm.FarBuffer(r.pcm_samples * 2)
        flat = pcm.t.view(torch.int16)
        _replicate(flat, lay._up(unit), po_, counts)
        for g in groups:
            for c, a in enumerate(host):
                pcm.put(int(po_[g + c]) * 2, a)
        adpcm, dec = fm.FarBuffer(r.adpcm_bytes), fm.FarBuffer(r.pcm_samples * 2)
        ws = torch.empty(max(r.workspace_bytes, 16), dtype=torch.uint8, device="cuda")
        coefs = torch.full((nch, 16), SENTINEL, dtype=torch.int16, device="cuda")
        status = torch.zeros(4, dtype=torch.int32, device="cuda")
        _ok(L.vga_gcadpcm_coefs_device_v(r.handle, pcm.ptr, coefs.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        _ok(L.vga_gcadpcm_encode_device_v(r.handle, pcm.ptr, coefs.data_ptr(), None, None, adpcm.ptr, _stream()))
        _ok(L.vga_gcadpcm_decode_device_v(r.handle, adpcm.ptr, coefs.data_ptr(), None, None, dec.ptr, status.data_ptr(), _stream()))
        torch.cuda.synchronize()
        assert status.cpu().numpy().tolist() == [0, 0, 0, 0]
        # unit 0 and every probe against the oracle
        got_coefs = coefs.cpu().numpy()
        checked = [(0, unit)] + [(g + c, a) for g in groups for c, a in enumerate(host)]
        for ch, x in checked:
            wc = po.gc_calculate_coefficients(x)
            wa = po.gc_encode(x, wc)
            _eq(got_coefs[ch], np.asarray(wc, np.int16).reshape(16), f"coefs of channel {ch}")
            _eq(adpcm.get(int(ao[ch]), len(wa)), np.asarray(wa, U8), f"adpcm of channel {ch} ({len(x)} samples)")
            _eq(dec.get(int(po_[ch]) * 2, len(x) * 2, np.int16), po.gc_decode(wa, wc, len(x)), f"decoded pcm of channel {ch}")
        # every other ballast unit against unit 0, on the device
        ballast = torch.from_numpy(np.flatnonzero(np.asarray(counts) == UNIT)).cuda()
        assert bool((coefs[ballast] == coefs[0]).all()), "coefficients of a ballast unit differ from unit 0's"
        _ballast_equal(adpcm.t, ao, counts, nb_unit, "adpcm")
        _ballast_equal(dec.t.view(torch.int16), po_, counts, UNIT, "decoded pcm")
        # nothing outside the rows' slots
        up = lay._round_up
        first = adpcm.untouched([(int(o), up(int(n), 16)) for o, n in zip(ao, r.byte_counts)])
        assert first is None, ("adpcm", adpcm.changed, first)
        first = dec.untouched([(int(o) * 2, up(int(n) * 2, 16)) for o, n in zip(po_, counts)])
        assert first is None, ("decoded pcm", dec.changed, first)
        first = pcm.untouched([(int(o) * 2, int(n) * 2) for o, n in zip(po_, counts)])
        assert first is None, ("the input pcm changed", pcm.changed, first)
        _eq(pcm.get(0, UNIT * 2, np.int16), unit, "the input's unit 0")
        _ballast_equal(flat, po_, counts, UNIT, "input pcm")
        # ---- the same rows as the channels of mono DSP files: channel metadata, the images, the images read back
        del flat, ws
        fm.release(pcm)
        pcm = None
        _gc_files_over_the_rows(r, counts, groups, checked, adpcm, dec, coefs)
        # ---- and as the channels of mono BRSTM files: the loop alignment (a copy-through here), the images, read back
        fm.release(dec)
        dec = None
        _nw_files_over_the_rows(r, counts, groups, checked, adpcm, coefs)
    finally:
        r.close()
        fm.release(pcm, adpcm, dec)


def _nw_files_over_the_rows(r, counts, groups, checked, adpcm, coefs):
    """vga_gcadpcm_align_channels_device_v, vga_nwstm_write_device_v and vga_nwstm_read_device_v on a vga_nw_files set (BRSTM,
    the default configuration) and its aligned set over the channels of test_gc_packed_chain, one mono file each.  The ballast
    files loop from sample 3 x 14336 and the longest probe from 14336, multiples of the alignment, so no channel is
    re-encoded and the aligned rows are copies; the other probes do not loop.  Unit 0 and the probes: rows, seek tables and
    loop contexts against the oracle's gc_build_channel, images against nwstm_ref's writer"""
    import nw_files_cases as nf
    from vgaudio_amd import _lib
    from vgaudio_amd.gcadpcm import AlignedFileSet
    from vgaudio_amd.nwstm import NwFileSet
    torch = _torch()
    L = _L()
    po = _po()
    cfg = nf.config(nf.RSTM)
    files = {n: nf.nw_file(1, n, 1, 14336 * 3, n) if n == UNIT else nf.nw_file(1, n, 1, 14336, n) if n > 14336 else nf.nw_file(1, n)
             for n in set(counts)}
    lays = {n: nf.file_layout(f, cfg)[1] for n, f in files.items()}
    assert all(l.alignment_needed == 0 and l.channel_sample_count == n for n, l in lays.items())
    s = NwFileSet([files[n] for n in counts], configuration=cfg)
    al = AlignedFileSet(s.gc_files())
    rs = out = seek = images = back = None
    try:
        nch, t, tot = s.channels, s.totals, al.totals
        i64p = C.POINTER(C.c_int64)
        pin, ain = al.offsets("in")
        _, aout = al.offsets("out")
        assert tot.aligned_channels == 0 and np.array_equal(ain, r.adpcm_offsets) and tot.adpcm_bytes <= adpcm.extent
        assert tot.out_adpcm_bytes == t.adpcm_bytes and np.array_equal(al.seek_offsets, s.seek_offsets) and tot.seek_shorts == t.seek_shorts
        io, so = s.image_offsets, s.seek_offsets
        for m in MARKS:
            # (an image is 1.4 KB longer than its row: behind 1800 of them the group lies in the second unit behind the mark)
            assert any(m <= int(io[g]) < m + 2 * lays[UNIT].file_size + (1 << 20) for g in groups), (m, [int(io[g]) for g in groups])
        wsb = max(int(tot.workspace_bytes), 16)
        fm.need(tot.out_adpcm_bytes * 2 + t.image_bytes + t.seek_shorts * 2 + wsb)
        out, seek, images = fm.FarBuffer(tot.out_adpcm_bytes), fm.FarBuffer(max(t.seek_shorts * 2, 16)), fm.FarBuffer(t.image_bytes)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        ctx = _i16_out(nch * 3)
        status = torch.zeros(2, dtype=torch.int32, device="cuda")
        is_unit = np.asarray(counts) == UNIT
        # (by length, not by channel: the read set below gets one parsed header per length, and its per-channel arrays are the
        # headers' it was made from)
        by_len = np.asarray(counts, np.int64)
        gain = np.where(is_unit, -9, by_len % 90 + 11).astype(np.int16)
        start = np.where(is_unit[:, None], (6, 7, -8), (by_len[:, None] * 3 + np.arange(3)) % 40 - 15).astype(np.int16)
        d_gain, d_start = lay._up(gain), lay._up(start)
        _ok(L.vga_gcadpcm_align_channels_device_v(al._h, adpcm.ptr, coefs.data_ptr(), out.ptr, None, seek.ptr, ctx.data_ptr(), status.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), _stream()))
        _ok(L.vga_nwstm_write_device_v(s._h, out.ptr, coefs.data_ptr(), d_gain.data_ptr(), d_start.data_ptr(), ctx.data_ptr(), seek.ptr,
                                       images.ptr, _stream()))
        torch.cuda.synchronize()
        assert status.cpu().numpy().tolist() == [0, 0]
        del ws
        got_coefs = coefs.cpu().numpy()
        got_ctx = ctx.cpu().numpy()
        assert np.all(got_ctx[nch * 3:] == SENTINEL)
        got_ctx = got_ctx[:nch * 3].reshape(nch, 3)
        assert np.all(got_ctx[is_unit] == got_ctx[0]), "loop context of a ballast unit differs from unit 0's"
        infos, seeks = {}, {}
        for ch, x in checked:
            n = len(x)
            c, wc = lays[n].channel, got_coefs[ch]
            wa = adpcm.get(int(ain[ch]), int(r.byte_counts[ch]))           # (held to the oracle by the chain)
            rc, _, a_out, _, wsk, wctx = po.gc_build_channel(wa, wc, po.gc_channel_params(c.sample_count, bool(c.looping), c.loop_start, c.loop_end,
                                                                                          c.loop_alignment_multiple, c.samples_per_seek_table_entry))
            assert rc == 0 and np.array_equal(a_out, wa)               # a copy-through
            _eq(out.get(int(aout[ch]), a_out.size), a_out, f"aligned row of channel {ch}")
            _eq(seek.get(int(so[ch]) * 2, wsk.size * 2, np.int16), wsk, f"seek table of channel {ch}")
            _eq(got_ctx[ch], wctx, f"loop context of channel {ch}")
            want = nf.reference_image(files[n], cfg, lays[n], [{"out": a_out, "coefs": wc, "seek": wsk}], [int(gain[ch])], [start[ch].tolist()],
                                      [got_ctx[ch].tolist()])
            want = np.frombuffer(bytes(want), U8)
            assert want.size == lays[n].file_size
            _eq(images.get(int(io[ch]), want.size), want, f"image of file {ch} ({n} samples)")
            img = np.ascontiguousarray(want)
            infos[n] = _lib.NwInfoC()
            _ok(L.vga_nwstm_parse(img.ctypes.data_as(_lib.u8p), img.size, C.byref(infos[n])))
            seeks[n] = wsk.size
        _ballast_equal(out.t, aout, counts, int(r.byte_counts[0]), "aligned rows")
        _ballast_equal(seek.t.view(torch.int16), so, counts, seeks[UNIT], "seek tables")
        _ballast_equal(images.t, io, counts, lays[UNIT].file_size, "images")
        first = out.untouched([(int(o), lay._round_up(int(n), 16)) for o, n in zip(aout, r.byte_counts)])
        assert first is None, ("aligned rows", out.changed, first)
        first = seek.untouched([(int(o) * 2, seeks[n] * 2) for o, n in zip(so, counts)])
        assert first is None, ("seek tables", seek.changed, first)
        first = images.untouched([(int(o), lays[n].file_size) for o, n in zip(io, counts)])
        assert first is None, ("images", images.changed, first)
        # the images read back through a set made from their parsed headers, at the writer's offsets
        rs = NwFileSet.from_infos([infos[n] for n in counts], [int(o) for o in io])
        rp, ra = np.zeros(nch, np.int64), np.zeros(nch, np.int64)
        _ok(L.vga_gcadpcm_ragged_offsets(rs.ragged, rp.ctypes.data_as(i64p), ra.ctypes.data_as(i64p)))
        back = fm.FarBuffer(rs.totals.adpcm_bytes)
        coefs2, gain2, start2, loop2 = _i16_out(nch * 16), _i16_out(nch), _i16_out(nch * 3), _i16_out(nch * 3)
        _ok(L.vga_nwstm_read_device_v(rs._h, images.ptr, back.ptr, coefs2.data_ptr(), gain2.data_ptr(), start2.data_ptr(), loop2.data_ptr(),
                                      _stream()))
        torch.cuda.synchronize()
        rows = [int(infos[n].adpcm_bytes) for n in counts]
        assert rows == [int(b) for b in r.byte_counts]
        for ch, x in checked:
            _eq(back.get(int(ra[ch]), rows[ch]), out.get(int(aout[ch]), rows[ch]), f"row {ch} read back")
        _ballast_equal(back.t, ra, counts, rows[0], "rows read back")
        first = back.untouched([(int(o), n) for o, n in zip(ra, rows)])
        assert first is None, ("rows read back", back.changed, first)
        _i16_is(coefs2, got_coefs, "coefficients read back")
        _i16_is(gain2, gain, "gains read back")
        _i16_is(start2, start, "start contexts read back")
        # (as test_gpu_nw_files.py: the loop context the parsed header holds -- the writer's, where the file loops)
        parsed = {n: np.array(list(infos[n].loop_context[0]), np.int16) for n in infos}
        assert all(np.array_equal(parsed[n], got_ctx[counts.index(n)]) for n in infos if lays[n].looping)
        _i16_is(loop2, np.stack([parsed[n] for n in counts]), "loop contexts read back")
    finally:
        al.close()
        s.close()
        if rs is not None:
            rs.close()
        fm.release(out, seek, images, back)


def _gc_files_over_the_rows(r, counts, groups, checked, adpcm, dec, coefs):
    """vga_gcadpcm_build_channels_device_v, vga_dsp_write_device_v and vga_dsp_read_device_v on a vga_gc_files set whose
    files are the channels of test_gc_packed_chain, one mono file each: the set's rows are the batch's rows, its packed
    images pass 2^31 and 2^32 where the ADPCM does.  adpcm: the encoder's output; dec: refilled, receives the set's PCM"""
    import gc_files_cases as gf
    from vgaudio_amd import _lib
    from vgaudio_amd import dsp as vdsp
    torch = _torch()
    L = _L()
    po = _po()
    spacing, spi = 14 * 64, 0x3800
    s = vdsp.DspFileSet([gf.gc_file(1, n, 0, 0, 0, spacing) for n in counts], gf.config(spi, 1, 1))
    rs = seek = images = back = None
    try:
        nch, t = s.channels, s.totals
        i64p = C.POINTER(C.c_int64)
        sp, sa = np.zeros(nch, np.int64), np.zeros(nch, np.int64)
        _ok(L.vga_gcadpcm_ragged_offsets(s.ragged, sp.ctypes.data_as(i64p), sa.ctypes.data_as(i64p)))
        assert np.array_equal(sp, r.pcm_offsets) and np.array_equal(sa, r.adpcm_offsets) and t.adpcm_bytes == r.adpcm_bytes
        io, so = s.image_offsets, s.seek_offsets
        for m in MARKS:
            assert any(m <= int(io[g]) < m + r.byte_counts[0] + (1 << 20) for g in groups), (m, [int(io[g]) for g in groups])
        fm.need(t.image_bytes + t.adpcm_bytes + t.seek_shorts * 2)
        dec.t.fill_(dec.fill)
        seek, images = fm.FarBuffer(max(t.seek_shorts * 2, 16)), fm.FarBuffer(t.image_bytes)
        ctx = _i16_out(nch * 3)
        status = torch.zeros(2, dtype=torch.int32, device="cuda")
        is_unit = np.asarray(counts) == UNIT
        gain = np.where(is_unit, 5, np.arange(nch) % 100 + 7).astype(np.int16)
        start = np.where(is_unit[:, None], (3, -4, 5), np.arange(nch * 3).reshape(nch, 3) % 50 - 20).astype(np.int16)
        start[:, 0] = adpcm.t[torch.from_numpy(sa).cuda()].cpu().numpy()          # (the frame header a start context begins with)
        d_gain, d_start, d_loop = lay._up(gain), lay._up(start), torch.zeros(nch * 3, dtype=torch.int16, device="cuda")
        _ok(L.vga_gcadpcm_build_channels_device_v(s._h, adpcm.ptr, coefs.data_ptr(), dec.ptr, seek.ptr, ctx.data_ptr(), status.data_ptr(), None, 0,
                                                  _stream()))
        _ok(L.vga_dsp_write_device_v(s._h, adpcm.ptr, coefs.data_ptr(), d_gain.data_ptr(), d_start.data_ptr(), d_loop.data_ptr(), images.ptr,
                                     _stream()))
        torch.cuda.synchronize()
        assert status.cpu().numpy().tolist() == [0, 0]
        got_coefs = coefs.cpu().numpy()
        got_ctx = ctx.cpu().numpy()
        assert np.all(got_ctx[nch * 3:] == SENTINEL)
        got_ctx = got_ctx[:nch * 3].reshape(nch, 3)
        assert np.all(got_ctx[is_unit] == got_ctx[0]), "loop context of a ballast unit differs from unit 0's"
        infos, sizes, seeks = {}, {}, {}
        for ch, x in checked:
            n = len(x)
            wc = got_coefs[ch]                                       # (held to the oracle above)
            wa = adpcm.get(int(sa[ch]), int(r.byte_counts[ch]))
            rc, _, _, wp, wsk, wctx = po.gc_build_channel(wa, wc, po.gc_channel_params(n, False, 0, 0, 0, spacing))
            assert rc == 0
            _eq(got_ctx[ch], wctx, f"loop context of channel {ch}")
            _eq(dec.get(int(sp[ch]) * 2, n * 2, np.int16), wp[:n], f"the set's pcm of channel {ch}")
            _eq(seek.get(int(so[ch]) * 2, wsk.size * 2, np.int16), wsk, f"seek table of channel {ch}")
            rc, img = po.dsp_write([wa], wc.reshape(1, 16), po.dsp_params(gf.RATE, n, False, 0, 0, spi, 1, True), gain=gain[ch:ch + 1],
                                   start_context=start[ch:ch + 1], loop_context=np.zeros((1, 3), np.int16))
            assert rc == 0 and img.size == s.image_sizes[ch]
            _eq(images.get(int(io[ch]), img.size), np.asarray(img, U8), f"image of file {ch} ({n} samples)")
            infos[n], sizes[n], seeks[n] = vdsp.parse(img.tobytes()), img.size, wsk.size
        _ballast_equal(dec.t.view(torch.int16), sp, counts, UNIT, "the set's pcm")
        _ballast_equal(seek.t.view(torch.int16), so, counts, seeks[UNIT], "seek tables")
        _ballast_equal(images.t, io, counts, sizes[UNIT], "images")
        first = images.untouched([(int(o), sizes[n]) for o, n in zip(io, counts)])
        assert first is None, ("images", images.changed, first)
        first = seek.untouched([(int(o) * 2, seeks[n] * 2) for o, n in zip(so, counts)])
        assert first is None, ("seek tables", seek.changed, first)
        first = dec.untouched([(int(o) * 2, lay._round_up(int(n) * 2, 16)) for o, n in zip(sp, counts)])
        assert first is None, ("the set's pcm", dec.changed, first)
        # the images read back through a set made from their parsed headers, at the writer's offsets
        rs = vdsp.DspFileSet.from_infos([infos[n] for n in counts], [int(o) for o in io])
        rp, ra = np.zeros(nch, np.int64), np.zeros(nch, np.int64)
        _ok(L.vga_gcadpcm_ragged_offsets(rs.ragged, rp.ctypes.data_as(i64p), ra.ctypes.data_as(i64p)))
        assert np.array_equal(ra, sa) and rs.totals.adpcm_bytes == t.adpcm_bytes
        back = fm.FarBuffer(rs.totals.adpcm_bytes)
        coefs2, gain2, start2, loop2 = _i16_out(nch * 16), _i16_out(nch), _i16_out(nch * 3), _i16_out(nch * 3)
        _ok(L.vga_dsp_read_device_v(rs._h, images.ptr, back.ptr, coefs2.data_ptr(), gain2.data_ptr(), start2.data_ptr(), loop2.data_ptr(),
                                    _stream()))
        torch.cuda.synchronize()
        for ch, x in checked:
            nb = int(r.byte_counts[ch])
            _eq(back.get(int(ra[ch]), nb), adpcm.get(int(sa[ch]), nb), f"row {ch} read back")
        _ballast_equal(back.t, ra, counts, int(r.byte_counts[0]), "rows read back")
        first = back.untouched([(int(o), int(n)) for o, n in zip(ra, r.byte_counts)])
        assert first is None, ("rows read back", back.changed, first)
        _i16_is(coefs2, got_coefs, "coefficients read back")
        _i16_is(gain2, gain, "gains read back")
        _i16_is(start2, start, "start contexts read back")
        _i16_is(loop2, np.zeros(nch * 3, np.int16), "loop contexts read back")
    finally:
        s.close()
        if rs is not None:
            rs.close()
        fm.release(seek, images, back)


@pytest.mark.gpu
def test_adx_packed_chain():
    """vga_adx_encode_device_v and vga_adx_decode_device_v (default parameters, 18-byte frames) on one batch whose packed
    PCM and packed ADX rows both pass 2^31 and 2^32 bytes: the histories and status words too"""
    from vgaudio_amd import _lib
    from vgaudio_amd.criadx import RaggedAdx
    torch = _torch()
    L = _L()
    po = _po()
    op = po.adx_params()
    nb_unit = -(-UNIT // 32) * 18
    counts, groups = _ballast_plan((lay._round_up(UNIT, 8) * 2, lay._round_up(nb_unit, 16)))
    r = RaggedAdx(_lib.AdxParams.from_buffer_copy(op), counts)
    pcm = adx = dec = None
    try:
        nch, t = r.channels, r.totals
        po_, ao = r.pcm_offsets, r.adx_offsets
        firsts = [int(po_[g]) * 2 for g in groups] + [int(ao[g]) for g in groups]
        for m in MARKS:
            room = 1 << 20
            assert any(m <= f < m + (1 << 23) + room for f in firsts[:len(groups)]) and any(m <= f < m + nb_unit + room for f in firsts[len(groups):])
        wsb = max(t.encode_workspace_bytes, t.decode_workspace_bytes, 16)
        need = t.pcm_samples * 4 + t.adx_bytes + wsb
        assert need < 46 * GIB, need
        fm.need(need)
        host = [po.synth_generate(1, n, first_channel=900 + c)[0] for c, n in enumerate(PROBES)]
        unit = po.synth_generate(1, UNIT, first_channel=899)[0]
        pcm = fm.FarBuffer(t.pcm_samples * 2)
        flat = pcm.t.view(torch.int16)
        _replicate(flat, lay._up(unit), po_, counts)
        for g in groups:
            for c, a in enumerate(host):
                pcm.put(int(po_[g + c]) * 2, a)
        adx, dec = fm.FarBuffer(t.adx_bytes), fm.FarBuffer(t.pcm_samples * 2)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        hist = torch.full((nch,), SENTINEL, dtype=torch.int16, device="cuda")
        status = torch.zeros(nch, dtype=torch.int32, device="cuda")
        _ok(L.vga_adx_encode_device_v(r._h, pcm.ptr, adx.ptr, hist.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        _ok(L.vga_adx_decode_device_v(r._h, adx.ptr, dec.ptr, ws.data_ptr(), ws.numel(), status.data_ptr(), _stream()))
        torch.cuda.synchronize()
        assert int(torch.count_nonzero(status)) == 0
        got_hist = hist.cpu().numpy()
        sizes = []
        for ch, x in [(0, unit)] + [(g + c, a) for g in groups for c, a in enumerate(host)]:
            wa, wh = po.adx_encode_batch(x[None, :], op)
            wa = np.asarray(wa, U8)[0]
            _eq(adx.get(int(ao[ch]), len(wa)), wa, f"adx of channel {ch} ({len(x)} samples)")
            assert int(got_hist[ch]) == int(np.asarray(wh).reshape(-1)[0]), ("history_out", ch)
            _eq(dec.get(int(po_[ch]) * 2, len(x) * 2, np.int16), np.asarray(po.adx_decode_batch(wa[None, :], len(x), op))[0], f"decoded pcm of channel {ch}")
        ballast = torch.from_numpy(np.flatnonzero(np.asarray(counts) == UNIT)).cuda()
        assert bool((hist[ballast] == hist[0]).all()), "history_out of a ballast unit differs from unit 0's"
        _ballast_equal(adx.t, ao, counts, nb_unit, "adx")
        _ballast_equal(dec.t.view(torch.int16), po_, counts, UNIT, "decoded pcm")
        up = lay._round_up
        sizes = [-(-int(n) // 32) * 18 for n in counts]
        first = adx.untouched([(int(o), up(n, 16)) for o, n in zip(ao, sizes)])
        assert first is None, ("adx", adx.changed, first)
        first = dec.untouched([(int(o) * 2, up(int(n) * 2, 16)) for o, n in zip(po_, counts)])
        assert first is None, ("decoded pcm", dec.changed, first)
        first = pcm.untouched([(int(o) * 2, int(n) * 2) for o, n in zip(po_, counts)])
        assert first is None, ("the input pcm changed", pcm.changed, first)
        _eq(pcm.get(0, UNIT * 2, np.int16), unit, "the input's unit 0")
        _ballast_equal(flat, po_, counts, UNIT, "input pcm")
        # ---- the same rows as the audio of mono ADX files: the images written, and read back
        del flat, ws
        fm.release(pcm, dec)
        pcm = dec = None
        _adx_files_over_the_rows(r, counts, groups, [(0, unit)] + [(g + c, a) for g in groups for c, a in enumerate(host)], adx, hist)
    finally:
        r.close()
        fm.release(pcm, adx, dec)


def _adx_files_over_the_rows(r, counts, groups, checked, adx, hist):
    """vga_adx_write_device_v and vga_adx_read_device_v on a vga_adx_files set whose files are the channels of
    test_adx_packed_chain, one mono version-4 file each, rows and images packed by the set itself: the set's rows are the
    ragged object's rows as they lie, and its packed images pass 2^31 and 2^32 where the ADX rows do.  Unit 0's and the
    probes' images are the oracle's AdxWriter's; the rows read back are the rows written"""
    import adx_files_cases as ac
    import test_gpu_adx_files as ta
    from vgaudio_amd import adx as vadx
    torch = _torch()
    L = _L()
    po = _po()
    files = {n: ac.adx_file((1, n, 0, 0, 0) + ac.D) for n in set(counts)}
    s = vadx.AdxFileSet([files[n] for n in counts])
    rs = images = back = None
    try:
        nch, t = s.channels, s.totals
        ao, io = r.adx_offsets, s.image_offsets
        assert np.array_equal(s.audio_offsets, ao) and t.audio_bytes <= adx.extent
        for m in MARKS:
            assert any(m <= int(io[g]) < m + (-(-UNIT // 32) * 18) + (1 << 20) for g in groups), (m, [int(io[g]) for g in groups])
        fm.need(t.image_bytes + t.audio_bytes)
        images = fm.FarBuffer(t.image_bytes)
        _ok(L.vga_adx_write_device_v(s._h, adx.ptr, hist.data_ptr(), images.ptr, _stream()))
        torch.cuda.synchronize()
        got_hist = hist.cpu().numpy()
        infos, sizes = {}, {}
        for ch, x in checked:
            n = len(x)
            row = adx.get(int(ao[ch]), ac.row_bytes(files[n]))               # (held to the oracle by the chain)
            rc, img = po.adxfile_write([row], got_hist[ch:ch + 1], ta.oracle_params(files[n].params))
            assert rc == 0
            _eq(images.get(int(io[ch]), img.size), np.asarray(img, U8), f"image of file {ch} ({n} samples)")
            infos[n], sizes[n] = vadx.parse(img.tobytes()), img.size
        _ballast_equal(images.t, io, counts, sizes[UNIT], "images")
        first = images.untouched([(int(o), sizes[n]) for o, n in zip(io, counts)])
        assert first is None, ("images", images.changed, first)
        # read back through a set made from the parsed headers, at the writer's offsets
        rs = vadx.AdxFileSet.from_infos([infos[n] for n in counts], [int(o) for o in io])
        assert np.array_equal(rs.audio_offsets, ao)
        back = fm.FarBuffer(rs.totals.audio_bytes)
        hist2 = _i16_out(nch)
        _ok(L.vga_adx_read_device_v(rs._h, images.ptr, back.ptr, hist2.data_ptr(), _stream()))
        torch.cuda.synchronize()
        rows = [ac.row_bytes(files[n]) for n in counts]
        for ch, x in checked:
            _eq(back.get(int(ao[ch]), rows[ch]), adx.get(int(ao[ch]), rows[ch]), f"row {ch} read back")
        _ballast_equal(back.t, ao, counts, rows[0], "rows read back")
        first = back.untouched([(int(o), n) for o, n in zip(ao, rows)])
        assert first is None, ("rows read back", back.changed, first)
        _i16_is(hist2, got_hist, "start histories read back")
    finally:
        s.close()
        if rs is not None:
            rs.close()
        fm.release(images, back)


@pytest.mark.gpu
def test_hca_packed_chain():
    """vga_hca_encode_device_v and vga_hca_decode_device_v on mono streams of the Highest quality (512-byte frames: of the
    qualities the one whose packed frames pass 2^32 bytes with the least PCM, 16 GiB of it)"""
    from vgaudio_amd import _lib
    from vgaudio_amd.crihca import RaggedHca
    torch = _torch()
    L = _L()
    po = _po()

    def info_of(n):
        p = po.hca_params(1, n, quality="Highest")
        cp = _lib.HcaParamsC(*[getattr(p, f) for f, _ in po.HcaParams._fields_])
        info = _lib.HcaInfoC()
        _ok(L.vga_hca_encoder_initialize(C.byref(cp), C.byref(info)))
        return p, info

    _, unit_info = info_of(UNIT)
    fb_unit = unit_info.frame_size * unit_info.frame_count
    counts, groups = _ballast_plan((lay._round_up(UNIT, 8) * 2, lay._round_up(fb_unit, 4)))
    made = {n: info_of(n) for n in set(counts)}
    r = RaggedHca([made[n][1] for n in counts])
    pcm = frames = dec = None
    try:
        t, fo, ro = r.totals, r.frame_offsets, r.pcm_row_offsets
        firsts = [int(ro[g]) * 2 for g in groups] + [int(fo[g]) for g in groups]
        for m in MARKS:
            room = 1 << 20
            assert any(m <= f < m + (1 << 23) + room for f in firsts[:len(groups)]) and any(m <= f < m + fb_unit + room for f in firsts[len(groups):])
        wsb = max(t.decode_workspace_bytes, 16)
        need = t.pcm_samples * 4 + t.frame_bytes + wsb
        assert need < 46 * GIB, need
        fm.need(need)
        host = [po.synth_generate(1, n, first_channel=900 + c)[0] for c, n in enumerate(PROBES)]
        unit = po.synth_generate(1, UNIT, first_channel=899)[0]
        pcm = fm.FarBuffer(t.pcm_samples * 2)
        flat = pcm.t.view(torch.int16)
        _replicate(flat, lay._up(unit), ro, counts)
        for g in groups:
            for c, a in enumerate(host):
                pcm.put(int(ro[g + c]) * 2, a)
        frames, dec = fm.FarBuffer(t.frame_bytes), fm.FarBuffer(t.pcm_samples * 2)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        st_e, st_d = (torch.zeros(len(counts), dtype=torch.int32, device="cuda") for _ in range(2))
        _ok(L.vga_hca_encode_device_v(r._h, pcm.ptr, frames.ptr, st_e.data_ptr(), _stream()))
        _ok(L.vga_hca_decode_device_v(r._h, frames.ptr, dec.ptr, ws.data_ptr(), ws.numel(), st_d.data_ptr(), _stream()))
        torch.cuda.synchronize()
        assert int(torch.count_nonzero(st_e)) == 0 and int(torch.count_nonzero(st_d)) == 0
        sizes = [made[n][1].frame_size * made[n][1].frame_count for n in counts]
        for s, x in [(0, unit)] + [(g + c, a) for g in groups for c, a in enumerate(host)]:
            rc, oi, wf = po.hca_encode(x[None, :], made[len(x)][0])
            assert rc == 0 and wf.size == sizes[s]
            _eq(frames.get(int(fo[s]), wf.size), np.asarray(wf, U8).reshape(-1), f"frames of stream {s} ({len(x)} samples)")
            rc, want = po.hca_decode(oi, wf)
            assert rc == 0
            _eq(dec.get(int(ro[s]) * 2, len(x) * 2, np.int16), np.ascontiguousarray(want)[0], f"decoded pcm of stream {s}")
        _ballast_equal(frames.t, fo, counts, fb_unit, "frames")
        _ballast_equal(dec.t.view(torch.int16), ro, counts, UNIT, "decoded pcm")
        up = lay._round_up
        first = frames.untouched([(int(o), up(n, 4)) for o, n in zip(fo, sizes)])
        assert first is None, ("frames", frames.changed, first)
        first = dec.untouched([(int(o) * 2, up(int(n) * 2, 16)) for o, n in zip(ro, counts)])
        assert first is None, ("decoded pcm", dec.changed, first)
        first = pcm.untouched([(int(o) * 2, int(n) * 2) for o, n in zip(ro, counts)])
        assert first is None, ("the input pcm changed", pcm.changed, first)
        _eq(pcm.get(0, UNIT * 2, np.int16), unit, "the input's unit 0")
        _ballast_equal(flat, ro, counts, UNIT, "input pcm")
        # ---- the same frames as the streams of HCA files: the images written, and read back
        del flat, ws
        fm.release(pcm, dec)
        pcm = dec = None
        _hca_files_over_the_frames(r, counts, groups, [0] + [g + c for g in groups for c in range(len(PROBES))], made, frames)
    finally:
        r.close()
        fm.release(pcm, frames, dec)


def _hca_files_over_the_frames(r, counts, groups, checked, made, frames):
    """vga_hca_write_device_v and vga_hca_read_device_v on a vga_hca_files set whose files are the streams of
    test_hca_packed_chain, unkeyed, frames and images packed by the set itself: the set's streams are the ragged object's as
    they lie, and its packed images pass 2^31 and 2^32 where the frames do.  Unit 0's and the probes' images are the
    oracle's HcaWriter's; the frames read back are the frames written, and no CRC is bad"""
    import hca_files_cases as hc
    from vgaudio_amd import _lib
    from vgaudio_amd import hca as vhca
    torch = _torch()
    L = _L()
    po = _po()
    files = {n: _lib.HcaFileC(made[n][1], None, 1.0, 0, 0, -1) for n in set(counts)}
    s = vhca.HcaFileSet([files[n] for n in counts])
    rs = images = back = None
    try:
        t, fo, io = s.totals, r.frame_offsets, s.image_offsets
        assert np.array_equal(s.frame_offsets, fo) and t.frame_bytes <= frames.extent
        sizes = {n: made[n][1].frame_size * made[n][1].frame_count for n in set(counts)}
        for m in MARKS:
            assert any(m <= int(io[g]) < m + sizes[UNIT] + (1 << 20) for g in groups), (m, [int(io[g]) for g in groups])
        fm.need(t.image_bytes + t.frame_bytes)
        images = fm.FarBuffer(t.image_bytes)
        _ok(L.vga_hca_write_device_v(s._h, frames.ptr, images.ptr, _stream()))
        torch.cuda.synchronize()
        infos, image_size = {}, {}
        for st in checked:
            n = counts[st]
            body = frames.get(int(fo[st]), sizes[n])                     # (held to the oracle by the chain)
            rc, img = po.hcafile_write(hc.oracle_info(made[n][1]), body, None, 1.0, 0, False)
            assert rc == 0
            _eq(images.get(int(io[st]), img.size), np.asarray(img, U8), f"image of file {st} ({n} samples)")
            infos[n], image_size[n] = vhca.parse(img.tobytes()), img.size
        _ballast_equal(images.t, io, counts, image_size[UNIT], "images")
        first = images.untouched([(int(o), image_size[n]) for o, n in zip(io, counts)])
        assert first is None, ("images", images.changed, first)
        rs = vhca.HcaFileSet.from_infos([infos[n] for n in counts], [int(o) for o in io])
        assert np.array_equal(rs.frame_offsets, fo)
        back = fm.FarBuffer(rs.totals.frame_bytes)
        bad = torch.zeros(len(counts), dtype=torch.int32, device="cuda")
        _ok(L.vga_hca_read_device_v(rs._h, images.ptr, back.ptr, bad.data_ptr(), _stream()))
        torch.cuda.synchronize()
        assert int(torch.count_nonzero(bad)) == 0, "a frame the encoder wrote fails its CRC after write and read"
        for st in checked:
            nb = sizes[counts[st]]
            _eq(back.get(int(fo[st]), nb), frames.get(int(fo[st]), nb), f"frames of file {st} read back")
        _ballast_equal(back.t, fo, counts, sizes[UNIT], "frames read back")
        first = back.untouched([(int(o), lay._round_up(sizes[n], 4)) for o, n in zip(fo, counts)])
        assert first is None, ("frames read back", back.changed, first)
    finally:
        s.close()
        if rs is not None:
            rs.close()
        fm.release(images, back)


@pytest.mark.gpu
def test_nwwav_bank_read_from_far_files():
    """vga_nwwav_bank_create takes the caller's file_offsets, so vga_nwwav_bank_read_device is a call at caller's offsets:
    six wave and prefetch files of test_gpu_nwwav.py's generator (two of each codec) at any byte around 2^31, 2^32 and 2^33;
    the three packed outputs are the restatement's rows (nwwav_ref), as in test_gpu_container_layouts.py"""
    import nwwav_ref as ref
    from test_gpu_nwwav import host_order, make_bank
    from vgaudio_amd import _lib
    from vgaudio_amd.nwwav import NwWaveBank
    torch = _torch()
    L = _L()
    made = [make_bank(950 + 3 * kind + codec, 1, [300 + 70 * kind], kind=kind, codec=codec)[0] for kind, codec in
            ((0, 0), (1, 1), (2, 2), (3, 0), (4, 1), (0, 2))]
    near = NwWaveBank([img for img, _ in made])                     # the parsed infos and the layout of the outputs
    structs = [ref.read_image(img) for img in near.images]
    assert {s["codec"] for s in structs} == {0, 1, 2}
    offs = np.array(far_spots([[len(img)] for img in near.images], 3), np.int64)
    h = C.c_void_p()
    buf = None
    try:
        _ok(L.vga_nwwav_bank_create(near.infos, offs.ctypes.data_as(C.POINTER(C.c_int64)), len(near.images), C.byref(h)))
        total = int(L.vga_nwwav_bank_source_bytes(h))                  # (to the end of the last file's audio)
        assert 1 << 33 < total <= int(offs[-1]) + len(near.images[-1])
        total = int(offs[-1]) + len(near.images[-1])
        rows_off = np.zeros(near.channels, np.int64)
        ints = [np.zeros(near.channels, np.int32) for _ in range(4)]
        _ok(L.vga_nwwav_bank_rows(h, *(a.ctypes.data_as(C.POINTER(C.c_int)) for a in ints), rows_off.ctypes.data_as(C.POINTER(C.c_int64))))
        assert np.array_equal(rows_off, near.offsets)                # where the rows go does not depend on where the files lie
        pieces = [(int(o), np.frombuffer(img, U8)) for o, img in zip(offs, near.images)]
        buf, windows = _far_source(total, pieces)
        sizes = (int(near.pcm8_bytes), int(near.pcm16_samples) * 2, int(near.adpcm_bytes))       # by NwCodec
        assert all(sizes)
        outs = [_near_out(n) for n in sizes]
        want = [np.zeros(n, U8) for n in sizes]
        r = 0
        for s in structs:
            for c in range(s["nch"]):
                row = host_order(s, c)
                at = int(near.offsets[r]) * (2 if s["codec"] == ref.PCM16 else 1)
                want[s["codec"]][at:at + len(row)] = row
                r += 1
        _ok(L.vga_nwwav_bank_read_device(h, buf.ptr + LEAD, outs[2].data_ptr() + EXTRA, outs[1].data_ptr() + EXTRA, outs[0].data_ptr() + EXTRA,
                                         _stream()))
        torch.cuda.synchronize()
        for codec, what in enumerate(("pcm8", "pcm16", "adpcm")):
            _near_is(outs[codec], [(0, want[codec])], what)
        _unchanged(buf, windows, pieces, "files")
    finally:
        if h:
            L.vga_nwwav_bank_destroy(h)
        near.close()
        fm.release(buf)


NW_SET = [1, 2, 3, 4, 5, 7]               # of nw_files_cases.SMALL: one to three channels, loops that were aligned and not


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rstm", "cstm-2.1", "fstm-0.3-little"])
def test_nw_files_read_from_far_images(name):
    """vga_nw_files_create_from_infos with image_offsets (multiples of 8), vga_nwstm_read_device_v on the images
    test_gpu_nw_files.py holds to the reference's writers: every row is what vga_nwstm_read_device reads from that file
    alone at offset 0 -- as there --, the per-channel arrays are the parsed header's"""
    import test_gpu_nw_files as tn
    from vgaudio_amd.nwstm import NwFileSet
    torch = _torch()
    _, _, files = tn.written_images(name)
    files = [files[k] for k in NW_SET]
    infos = [tn.parse(f) for f in files]
    offs = far_spots([[len(f)] for f in files], 8)
    r = NwFileSet.from_infos(infos, offs)
    buf = None
    try:
        nch, tot = r.channels, r.totals
        assert list(r.image_offsets) == offs and tot.image_bytes > 1 << 33
        pieces = list(zip(offs, files))
        buf, windows = _far_source(tot.image_bytes, pieces)
        rows = _near_out(tot.adpcm_bytes)
        coefs, gain, start, loop = _i16_out(nch * 16), _i16_out(nch), _i16_out(nch * 3), _i16_out(nch * 3)
        _ok(_L().vga_nwstm_read_device_v(r._h, buf.ptr + LEAD, rows.data_ptr() + EXTRA, coefs.data_ptr(), gain.data_ptr(), start.data_ptr(),
                                         loop.data_ptr(), _stream()))
        torch.cuda.synchronize()
        _, ao = tn.row_offsets(r.ragged, nch)
        wanted, want, c = [], dict(coefs=[], gain=[], start=[], loop=[]), 0
        for f, info in zip(files, infos):
            k, n = info.channel_count, info.adpcm_bytes
            pitch = max(lay._round_up(n, 16), 16)
            own = torch.full((k, pitch), JUNK, dtype=torch.uint8, device="cuda")
            d_file = lay._up(f)
            _ok(_L().vga_nwstm_read_device(C.byref(info), d_file.data_ptr(), len(f), 1, own.data_ptr(), pitch, _stream()))
            torch.cuda.synchronize()
            own = own.cpu().numpy()
            for i in range(k):
                wanted.append((ao[c + i], own[i, :n].copy()))
                want["coefs"].append(list(info.coefs[i])), want["gain"].append(info.gain[i])
                want["start"].append(list(info.start_context[i])), want["loop"].append(list(info.loop_context[i]))
            c += k
        _near_is(rows, wanted, "rows")
        for t, key in ((coefs, "coefs"), (gain, "gain"), (start, "start"), (loop, "loop")):
            _i16_is(t, want[key], key)
        _unchanged(buf, windows, pieces, "images")
    finally:
        r.close()
        fm.release(buf)

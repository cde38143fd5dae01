"""include/vgaudio_hip_files/hca_keyed_files.h on the GPU: the keys the search finds against the oracle's FindKey per file
(index and status; images packed and at odd byte offsets; whatever the workspace held), every candidate singly against the
oracle's verdict, the chain search -> keyed read -> decode without a synchronisation in between, the keyed read byte for byte
against vga_hca_read_device_v on a set created with the same keys (both forms, the forced general form, bad-CRC counts) and
against the oracle's cipher; junk-filled buffers larger than needed with every byte outside the outputs checked; poison mode;
a busy caller stream; two streams at once; refused calls launch nothing; hca.read_files(Keys=...) against HcaReader per file.
The cases and every expectation are tests/hca_keyed_files_cases.py's, computed with the oracle alone."""
import ctypes as C

import numpy as np
import pytest

import hca_keyed_files_cases as kc
from oracle import pyoracle as po
from test_gpu_device_streams import delay  # noqa: F401  (the calibrated GPU delay that makes a caller's stream busy)
from vgaudio_amd import _lib
from vgaudio_amd import hca
from vgaudio_amd.crihca import CriHcaKey, RaggedHca
from vgaudio_amd.hca import HcaFileSet, HcaReader

pytestmark = pytest.mark.gpu

# function of the header -> the tests that call it
CASES = {
    "vga_hca_find_keys_workspace_bytes": ["test_found_keys_are_the_oracles", "test_refused_calls_launch_nothing"],
    "vga_hca_find_keys_device_v": [
        "test_found_keys_are_the_oracles", "test_every_candidate_singly_has_the_oracles_verdict", "test_find_read_decode_chain",
        "test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream", "test_two_streams_at_once",
        "test_refused_calls_launch_nothing", "test_read_files_with_keys_is_the_readers"],
    "vga_hca_read_keyed_device_v": [
        "test_keyed_read_is_the_read_with_create_time_keys", "test_find_read_decode_chain", "test_bytes_do_not_depend_on_poison",
        "test_calls_on_a_busy_stream", "test_two_streams_at_once", "test_refused_calls_launch_nothing",
        "test_read_files_with_keys_is_the_readers"],
    "vga_hca_find_keys_items_for": ["test_found_keys_are_the_oracles"],
}

JUNK = 0xEE
EXTRA = 64                                                             # junk in front of and behind every buffer (keeps 16-byte alignment)
POOL_STREAMS = 32                                                      # torch hands out this many streams, round robin
MARK = 0x55555555
NT = kc.NCODES + 1                                                     # tables of the keyed read: every code, then type 1


def torch():
    import torch as t
    return t


def L():
    return _lib.lib()


def last_error():
    return L().vga_last_error().decode("utf-8", "replace")


def dev(a):
    return torch().from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def stream_ptr(stream=None):
    t = torch()
    return C.c_void_p((stream if stream is not None else t.cuda.current_stream()).cuda_stream)


def all_tables():
    t = kc.table()
    return np.concatenate([t["dec"], t["dec1"][None, :]])


def d_tables(codes, odd=True):
    """the decryption tables of CODES[codes] and the type-1 table behind them on the device, at an odd byte when asked: (keep, view)"""
    t = kc.table()
    flat = np.concatenate([t["dec"][list(codes)].reshape(-1), t["dec1"]]).astype(np.uint8)
    keep = dev(np.concatenate([np.full(3 if odd else 0, JUNK, np.uint8), flat]))
    return keep, keep[3 if odd else 0:]


class ReadSet:
    """The table's files as one set for reading, created without keys; images packed or at odd byte offsets in a junk-filled buffer"""

    def __init__(self, offsets="packed", files=None, keys=None, tables=None, fill=JUNK):
        t = kc.table()
        self.which = list(range(len(kc.FILES))) if files is None else [kc.index_of(n) for n in files]
        self.infos = [t["infos"][n] for n in self.which]
        self.datas = [t["datas"][n] for n in self.which]
        offs = None
        if offsets == "odd":
            offs, at = [], 3
            for d in self.datas:
                offs.append(at)
                at += len(d) + 5 + (len(d) & 1)
        self.s = HcaFileSet.from_infos(self.infos, image_offsets=offs, keys=keys, tables=tables)
        self.packed = np.full(self.s.totals.image_bytes, fill, np.uint8)
        for d, at in zip(self.datas, self.s.image_offsets):
            self.packed[int(at):int(at) + len(d)] = np.frombuffer(d, np.uint8)
        self.n = len(self.which)

    def close(self):
        self.s.close()

    def frames(self, fill=JUNK):
        return torch().full((self.s.totals.frame_bytes + 2 * EXTRA,), fill, dtype=torch().uint8, device="cuda")

    def expected_frames(self, per_file, fill=JUNK):
        """the whole frames buffer: fill, and every stream followed by its zeros up to the next multiple of 4"""
        want = np.full(self.s.totals.frame_bytes + 2 * EXTRA, fill, np.uint8)
        for f, a in enumerate(per_file):
            a = np.asarray(a, np.uint8).reshape(-1)
            at = EXTRA + int(self.s.frame_offsets[f])
            want[at:at + len(a)] = a
            want[at + len(a):at + (len(a) + 3) // 4 * 4] = 0
        return want

    def read_keyed(self, d_images, frames, tables, index, bad=None, status=None, stream=None, ntables=None):
        check = _lib.check
        check(L().vga_hca_read_keyed_device_v(self.s._h, d_images.data_ptr(), tables.data_ptr(), tables.numel() // 256 if ntables is None else ntables,
                                              index.data_ptr() if index is not None else None, frames.data_ptr() + EXTRA,
                                              bad.data_ptr() if bad is not None else None, status.data_ptr() if status is not None else None,
                                              stream_ptr(stream)))

    def find(self, d_images, tables, nkeys, type1_index, workspace, stream=None, with_status=True):
        """(index out, status out), each nfiles + 8 ints of MARK"""
        t = torch()
        out = t.full((self.n + 8,), MARK, dtype=t.int32, device="cuda")
        status = t.full((self.n + 8,), MARK, dtype=t.int32, device="cuda")
        _lib.check(L().vga_hca_find_keys_device_v(self.s._h, d_images.data_ptr(), tables.data_ptr(), nkeys, type1_index, out.data_ptr(),
                                                  status.data_ptr() if with_status else None, workspace.data_ptr(), workspace.numel(),
                                                  stream_ptr(stream)))
        return out, status


def expected_found(rs, name):
    return [kc.table()["found"][name][n] for n in rs.which]


def check_found(rs, out, status, name, what):
    want = expected_found(rs, name)
    o, s = host(out), host(status)
    assert list(zip(o[:rs.n].tolist(), s[:rs.n].tolist())) == want, (what, [(kc.NAMES[rs.which[f]], g, w) for f, (g, w) in enumerate(
        zip(zip(o[:rs.n].tolist(), s[:rs.n].tolist()), want)) if g != w])
    assert np.all(o[rs.n:] == MARK) and np.all(s[rs.n:] == MARK), what


def crypt(stored, table):
    if stored.size == 0:
        return stored.reshape(-1)
    return po.hca_crypt(stored, stored.shape[1], table)


def expected_read(rs, index):
    """per file what the keyed read leaves under table indices `index` into all_tables(): (frames, status)"""
    t, tabs = kc.table(), all_tables()
    frames = [crypt(t["stored"][n], tabs[i]) if 0 <= i < NT else t["stored"][n].reshape(-1) for n, i in zip(rs.which, index)]
    return frames, [1 if i >= NT else 0 for i in index]


# ---------------------------------------------------------------- 1. the search
@pytest.mark.parametrize("name", sorted(kc.LISTS))
@pytest.mark.parametrize("offsets", ["packed", "odd"])
def test_found_keys_are_the_oracles(offsets, name):
    t = torch()
    codes = kc.LISTS[name]
    rs = ReadSet(offsets)
    try:
        items = [(i.file, i.first_key, i.key_count) for i in HcaFileSet.find_items(rs.infos, len(codes))]
        assert items == kc.find_items_model(kc.table()["types"], len(codes))
        need = rs.s.find_keys_workspace_bytes(len(codes))
        assert need == kc.workspace_model(rs.n, len(codes))
        d_images = dev(rs.packed)
        keep, tables = d_tables(codes, odd=offsets == "odd")
        before = host(keep).copy()
        results = []
        for fill in (0x00, 0xA5, 0xFF):
            workspace = t.full((need + EXTRA,), fill, dtype=t.uint8, device="cuda")
            out, status = rs.find(d_images, tables, len(codes), len(codes), workspace)
            t.cuda.synchronize()
            check_found(rs, out, status, name, (offsets, name, fill))
            assert np.all(host(workspace)[need:] == fill)
            results.append((host(out).tobytes(), host(status).tobytes()))
        assert results[0] == results[1] == results[2]
        # without d_status: the same indices
        out, status = rs.find(d_images, tables, len(codes), len(codes), workspace, with_status=False)
        t.cuda.synchronize()
        assert host(out).tobytes() == results[0][0] and np.all(host(status) == MARK)
        assert np.array_equal(host(d_images), rs.packed) and np.array_equal(host(keep), before)
    finally:
        rs.close()


def test_every_candidate_singly_has_the_oracles_verdict():
    """nkeys = 1 at d_tables + 256 * k: every candidate on the files made for wrong keys that pass, the first sixteen on the rest"""
    t = torch()
    rs = ReadSet("odd")
    try:
        single = kc.table()["single"]
        d_images = dev(rs.packed)
        keep, tables = d_tables(range(kc.NCODES))
        workspace = t.empty(rs.s.find_keys_workspace_bytes(1), dtype=t.uint8, device="cuda")
        outs = [rs.find(d_images, tables[256 * k:], 1, -1, workspace) for k in range(kc.NCODES)]
        t.cuda.synchronize()
        passes = 0
        for k, (out, status) in enumerate(outs):
            o, s = host(out), host(status)
            for f, n in enumerate(rs.which):
                if n in single and k < len(single[n]):
                    want = (0, 0) if single[n][k] == 0 else kc.verdict(single[n][k])
                    assert (o[f], s[f]) == want, (kc.NAMES[n], k)
                    passes += want == (0, 0)
        assert passes > 20
    finally:
        rs.close()


# ---------------------------------------------------------------- 2. the keyed read
@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("offsets", ["packed", "odd"])
def test_keyed_read_is_the_read_with_create_time_keys(offsets, general):
    t = torch()
    index = kc.read_key_indices()
    own_keys = [i if 0 <= i < NT else -1 for i in index]
    rs, own = ReadSet(offsets), ReadSet(offsets, keys=own_keys, tables=all_tables())
    old = L().vga_hca_files_force_general_this_thread(1 if general else 0)
    try:
        stats = rs.s.stats()
        assert (stats[0] == 0) == general and stats == own.s.stats()
        d_images = dev(rs.packed)
        keep, tables = d_tables(range(kc.NCODES))
        d_index = dev(np.array(index + [MARK], np.int32))
        want_frames, want_status = expected_read(rs, index)
        damaged = np.array(rs.packed, copy=True)                       # a bad CRC in two files, one keyed and one not
        for name in ("last", "type0"):
            f = rs.which.index(kc.index_of(name))
            damaged[int(rs.s.image_offsets[f]) + rs.infos[f].frames_offset + 7] ^= 0x40
        for images, with_bad in ((rs.packed, False), (rs.packed, True), (damaged, True)):
            d_images = dev(images)
            frames, ref = rs.frames(), own.frames()
            bad, ref_bad = (t.full((rs.n + 8,), 7, dtype=t.int32, device="cuda") for _ in range(2))
            status = t.full((rs.n + 8,), MARK, dtype=t.int32, device="cuda")
            rs.read_keyed(d_images, frames, tables, d_index, bad if with_bad else None, status)
            _lib.check(L().vga_hca_read_device_v(own.s._h, d_images.data_ptr(), ref.data_ptr() + EXTRA,
                                                 ref_bad.data_ptr() if with_bad else None, stream_ptr()))
            t.cuda.synchronize()
            assert np.array_equal(host(frames), host(ref)), (offsets, general, with_bad)
            assert np.array_equal(host(bad), host(ref_bad))
            stored_bad = np.array([kc.table()["bad_crc"][n] for n in rs.which])    # hand-made frames carry no valid CRC
            assert np.all(host(bad)[rs.n:] == 7)
            if images is rs.packed:
                assert np.array_equal(host(frames), rs.expected_frames(want_frames))
                assert np.array_equal(host(bad)[:rs.n] - 7, stored_bad if with_bad else 0 * stored_bad)
            else:
                more = host(bad)[:rs.n] - 7 - stored_bad
                assert more.sum() == 2 and more[rs.which.index(kc.index_of("last"))] == 1 and more.min() == 0
            assert list(host(status)[:rs.n]) == want_status and np.all(host(status)[rs.n:] == MARK)
            assert np.array_equal(host(d_images), images)
        # a null index is table 0 for every file
        frames = rs.frames()
        rs.read_keyed(d_images, frames, tables, None)
        t.cuda.synchronize()
        # (d_images holds the damaged copy: the stored bytes are what they are)
        t_ = kc.table()
        zero = [crypt(np.frombuffer(damaged[int(at) + i.frames_offset:int(at) + i.frames_offset + i.hca.frame_count * i.hca.frame_size].tobytes(),
                                    np.uint8).reshape(i.hca.frame_count, i.hca.frame_size), t_["dec"][0])
                for at, i in zip(rs.s.image_offsets, rs.infos)]
        assert np.array_equal(host(frames), rs.expected_frames(zero))
    finally:
        L().vga_hca_files_force_general_this_thread(old)
        rs.close()
        own.close()


CHAIN = ["type1", "last", "silent", "key63"]                          # one shape class: stereo, Low


def test_find_read_decode_chain():
    """search -> keyed read -> vga_hca_decode_device_v on one stream, nothing read on the host in between: the oracle's decode of
    the plain streams"""
    t = torch()
    table = kc.table()
    rs = ReadSet("odd", files=CHAIN)
    r = RaggedHca([i.hca for i in rs.infos])
    try:
        assert list(r.frame_offsets) == list(rs.s.frame_offsets) and r.totals.frame_bytes == rs.s.totals.frame_bytes
        codes = kc.LISTS["n65"]
        d_images = dev(rs.packed)
        keep, tables = d_tables(codes)
        workspace = t.empty(rs.s.find_keys_workspace_bytes(len(codes)), dtype=t.uint8, device="cuda")
        frames = t.full((r.totals.frame_bytes,), JUNK, dtype=t.uint8, device="cuda")
        pcm = t.zeros(max(r.totals.pcm_samples, 1), dtype=t.int16, device="cuda")
        dws = t.empty(max(r.totals.decode_workspace_bytes, 16), dtype=t.uint8, device="cuda")
        dstatus = t.zeros(r.streams, dtype=t.int32, device="cuda")
        index = rs.s.find_keys_device(d_images, tables, len(codes), type1_index=len(codes), workspace=workspace)
        rs.s.read_keyed_device(d_images, tables, frames, key_index=index)
        r.decode_device(frames, pcm, dws, dstatus)
        t.cuda.synchronize()
        assert list(host(index)) == [i for i, _ in expected_found(rs, "n65")] and not host(dstatus).any()
        flat, row = host(pcm), 0
        for f, n in enumerate(rs.which):
            rc, want = po.hca_decode(table["oinfo"][n], table["plain"][n])
            assert rc == 0
            for c in range(want.shape[0]):
                at = int(r.pcm_row_offsets[row])
                assert np.array_equal(flat[at:at + want.shape[1]], want[c]), (CHAIN[f], c)
                row += 1
    finally:
        r.close()
        rs.close()


# ---------------------------------------------------------------- 3. poison mode
@pytest.mark.parametrize("value", [0xA5, 0xFF])
def test_bytes_do_not_depend_on_poison(value):
    t = torch()
    old = L().vga_testing_poison_allocations(value)
    fill = value ^ 0x3C
    try:
        rs = ReadSet("packed", fill=value)                             # (created under the mode: its tables are poisoned first)
        try:
            d_images = dev(rs.packed)
            keep, tables = d_tables(range(kc.NCODES))
            index = kc.read_key_indices()
            frames = rs.frames(fill)
            rs.read_keyed(d_images, frames, tables, dev(np.array(index, np.int32)))
            workspace = t.full((rs.s.find_keys_workspace_bytes(kc.NCODES),), value, dtype=t.uint8, device="cuda")
            out, status = rs.find(d_images, tables, kc.NCODES, kc.NCODES, workspace)
            t.cuda.synchronize()
            assert np.array_equal(host(frames), rs.expected_frames(expected_read(rs, index)[0], fill))
            check_found(rs, out, status, "n130", ("poison", value))
        finally:
            rs.close()
    finally:
        t.cuda.synchronize()
        L().vga_testing_poison_allocations(old if old >= 0 else -1)


# ---------------------------------------------------------------- 4. streams
_streams = []


def some_streams(n):
    """Streams for this file, taken once and so that the files that run after it find torch's stream pool as they would without
    it (tests/test_gpu_nw_files.py: some_streams): one whole turn of the pool with the imported `delay` fixture's, every stream
    used once, in order."""
    t = torch()
    if not _streams:
        _streams.extend(t.cuda.Stream() for _ in range(POOL_STREAMS - 1))
        for s in _streams:
            with t.cuda.stream(s):
                t.zeros(1, device="cuda")
        t.cuda.synchronize()
    return _streams[:n]


def frames_under_found(rs, name):
    """what the keyed read leaves with the indices the search gives over LISTS[name] (type 1 behind the candidates)"""
    t, codes = kc.table(), kc.LISTS[name]
    tabs = np.concatenate([t["dec"][codes], t["dec1"][None, :]])
    return [crypt(t["stored"][n], tabs[i]) if i >= 0 else t["stored"][n].reshape(-1) for n, (i, _) in zip(rs.which, expected_found(rs, name))]


def test_calls_on_a_busy_stream(delay):  # noqa: F811
    """The chain search -> keyed read with the search's index tensor, queued behind a delay on the caller's stream: the calls do
    not wait for it and nothing reads the indices on the host; they are ordered after the delay -- their input is written on
    the same stream behind it"""
    t = torch()
    cycles, ms = delay
    rs = ReadSet("packed")
    try:
        (S,) = some_streams(1)
        codes = kc.LISTS["n65"]
        d_packed = dev(rs.packed)
        keep, tables = d_tables(codes)
        workspace = t.full((rs.s.find_keys_workspace_bytes(len(codes)),), 0x77, dtype=t.uint8, device="cuda")
        with t.cuda.stream(S):
            for busy in (False, True):                                 # (warm first: every kernel has run once)
                d_images, frames = t.zeros_like(d_packed), rs.frames()
                S.synchronize()
                if busy:
                    t.cuda._sleep(cycles)
                d_images.copy_(d_packed, non_blocking=True)            # the input arrives behind the delay
                out, status = rs.find(d_images, tables, len(codes), len(codes), workspace, stream=S)
                rs.read_keyed(d_images, frames, tables, out, stream=S)
                if busy:
                    assert not S.query(), "the caller's stream was idle when the calls returned (they waited for it)"
        S.synchronize()
        check_found(rs, out, status, "n65", "busy stream")
        assert np.array_equal(host(frames), rs.expected_frames(frames_under_found(rs, "n65")))
    finally:
        rs.close()


def test_two_streams_at_once():
    """one object, two streams"""
    t = torch()
    rs = ReadSet("odd")
    try:
        S1, S2 = some_streams(2)
        codes = kc.LISTS["n130"]
        d_images = dev(rs.packed)
        keep, tables = d_tables(codes)
        need = rs.s.find_keys_workspace_bytes(len(codes))
        w1, w2 = (t.full((need,), v, dtype=t.uint8, device="cuda") for v in (0, 0xFF))
        f1, f2 = rs.frames(), rs.frames(0x11)
        t.cuda.synchronize()
        o1, s1 = rs.find(d_images, tables, len(codes), len(codes), w1, stream=S1)
        o2, s2 = rs.find(d_images, tables, len(codes), len(codes), w2, stream=S2)
        rs.read_keyed(d_images, f1, tables, o1, stream=S1)
        rs.read_keyed(d_images, f2, tables, o2, stream=S2)
        S1.synchronize()
        S2.synchronize()
        check_found(rs, o1, s1, "n130", "stream 1")
        check_found(rs, o2, s2, "n130", "stream 2")
        want = frames_under_found(rs, "n130")
        assert np.array_equal(host(f1), rs.expected_frames(want))
        assert np.array_equal(host(f2), rs.expected_frames(want, 0x11))
    finally:
        rs.close()


# ---------------------------------------------------------------- 5. refused calls
def test_refused_calls_launch_nothing():
    t = torch()
    table = kc.table()
    rs, own = ReadSet("packed"), ReadSet("packed", keys=[-1] * len(kc.FILES), tables=all_tables())
    first = table["infos"][kc.index_of("first")]
    ws = HcaFileSet([_lib.HcaFileC(first.hca, None, 1.0, 0, 0, -1)])
    try:
        d_images, frames = dev(rs.packed), rs.frames()
        keep, tables = d_tables(range(kc.NCODES), odd=False)
        out = t.full((rs.n,), MARK, dtype=t.int32, device="cuda")
        status = t.full((rs.n,), MARK, dtype=t.int32, device="cuda")
        need = L().vga_hca_find_keys_workspace_bytes(rs.s._h, 12)
        assert need == kc.workspace_model(rs.n, 12) and L().vga_hca_find_keys_workspace_bytes(ws._h, 12) == 0
        workspace = t.full((need,), JUNK, dtype=t.uint8, device="cuda")
        fd, rd = L().vga_hca_find_keys_device_v, L().vga_hca_read_keyed_device_v
        st, sp = stream_ptr(), status.data_ptr()
        I, T, O, W, F = d_images.data_ptr(), tables.data_ptr(), out.data_ptr(), workspace.data_ptr(), frames.data_ptr() + EXTRA
        assert fd(ws._h, I, T, 12, -1, O, sp, W, need, st) == -4           # a set for writing
        assert rd(ws._h, I, T, NT, None, F, None, sp, st) == -4
        assert fd(own.s._h, I, T, 12, -1, O, sp, W, need, st) == -4        # a set with keys of its own
        assert rd(own.s._h, I, T, NT, None, F, None, sp, st) == -4
        assert "keys of its own" in last_error()
        assert fd(rs.s._h, I, T, -1, -1, O, sp, W, need, st) == -1
        assert fd(rs.s._h, I, T, 12, -2, O, sp, W, need, st) == -1
        assert fd(rs.s._h, I, None, 12, -1, O, sp, W, need, st) == -1
        assert fd(rs.s._h, I, T, 12, -1, None, sp, W, need, st) == -1
        assert fd(rs.s._h, None, T, 12, -1, O, sp, W, need, st) == -1
        assert fd(rs.s._h, I + 4, T, 12, -1, O, sp, W, need, st) == -1
        assert fd(rs.s._h, I, T, 12, -1, O, sp, None, need, st) == -1
        assert fd(rs.s._h, I, T, 12, -1, O, sp, W, need - 1, st) == -1
        assert fd(rs.s._h, I, T, 12, -1, O, sp, W + 2, need, st) == -1
        assert last_error().startswith("vga_hca_find_keys_device_v: ")
        # a type-56 file whose header the per-file search refuses (nine channels): the set is made, only the search refuses it
        nine = _lib.HcaFileInfoC.from_buffer_copy(first)
        nine.hca.channel_count = 9
        unusable = HcaFileSet.from_infos([nine])
        try:
            assert fd(unusable._h, I, T, 12, -1, O, sp, W, need, st) == -1
            assert "file 0: HcaInfo is inconsistent" in last_error() and last_error().startswith("vga_hca_find_keys_device_v: ")
        finally:
            unusable.close()
        assert rd(rs.s._h, I, None, NT, None, F, None, sp, st) == -1
        assert rd(rs.s._h, I, T, 0, None, F, None, sp, st) == -1
        assert rd(rs.s._h, I, T, -2, None, F, None, sp, st) == -1
        assert rd(rs.s._h, None, T, NT, None, F, None, sp, st) == -1
        assert rd(rs.s._h, I, T, NT, None, None, None, sp, st) == -1
        assert rd(rs.s._h, I + 1, T, NT, None, F, None, sp, st) == -1
        assert rd(rs.s._h, I, T, NT, None, F + 2, None, sp, st) == -1
        assert last_error().startswith("vga_hca_read_keyed_device_v: ")
        t.cuda.synchronize()
        assert np.all(host(frames) == JUNK) and np.all(host(workspace) == JUNK)
        assert np.all(host(out) == MARK) and np.all(host(status) == MARK)
    finally:
        ws.close()
        own.close()
        rs.close()


# ---------------------------------------------------------------- 6. the Python layer
READER_FILES = ["type0", "type1", "first", "middle", "last", "silent", "silent3", "short_tail", "key63", "key64", "no_frames"]


def test_read_files_with_keys_is_the_readers():
    table = kc.table()
    keys = [CriHcaKey(kc.CODES[k]) for k in kc.LISTS["n65"]]
    assert all(np.array_equal(k.DecryptionTable, table["dec"][i]) for i, k in enumerate(keys))
    datas = [table["datas"][kc.index_of(n)] for n in READER_FILES]
    formats, bad = hca.read_files(datas, Keys=keys)
    assert bad == [0] * len(datas)
    for name, data, fmt in zip(READER_FILES, datas, formats):
        want, _ = HcaReader(Keys=keys).ReadWithConfig(data)
        assert np.array_equal(fmt.AudioData, want.AudioData), name
        assert fmt.Hca.EncryptionType == want.Hca.EncryptionType and fmt.Hca.FrameCount == want.Hca.FrameCount, name
        n = kc.index_of(name)
        if table["types"][n] and len(table["plain"][n]):
            assert np.array_equal(fmt.AudioData, table["plain"][n]), name
    # the two errors, named by file, after the reader's own
    for name, message in (("absent", "Cannot find key to decrypt HCA file."), ("sync_with_key", "Invalid frame header")):
        data = table["datas"][kc.index_of(name)]
        with pytest.raises(_lib.InvalidDataError) as per_file:
            HcaReader(Keys=keys).ReadWithConfig(data)
        assert str(per_file.value) == message
        with pytest.raises(_lib.InvalidDataError) as e:
            hca.read_files(datas[:3] + [data] + datas[3:], Keys=keys)
        assert str(e.value) == "file 3: " + message
    # without Keys: as before
    with pytest.raises(_lib.InvalidDataError) as e:
        hca.read_files(datas)
    assert str(e.value) == "file 2: Cannot find key to decrypt HCA file."
    assert hca.read_files([], Keys=keys) == ([], [])

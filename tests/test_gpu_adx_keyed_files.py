"""include/vgaudio_hip_files/adx_keyed_files.h on the GPU: the keyed images of a set of ADX files against the oracle's AdxWriter
over encrypted rows and against vga_adx_crypt_device + vga_adx_write_device file by file, the keyed rows against the oracle's
AdxReader + EncryptDecrypt and against vga_adx_read_device + vga_adx_crypt_device, both inside junk-filled buffers whose every
byte outside the images / rows is checked; the search against the oracle's TestKey over each file's sub-list and against
vga_adx_find_key_device; search -> keyed read on a busy stream without touching the host; the forced general form; poison
mode; two streams at once; refused calls; adx.write_files / adx.read_files with keys against AdxWriter / AdxReader.  The cases
and every expectation are tests/adx_keyed_files_cases.py's (the oracle alone); tests/test_adx_keyed_files_host.py checks
that CASES names every function of the header."""
import ctypes as C

import numpy as np
import pytest

import adx_files_cases as ac
import adx_keyed_files_cases as kc
from oracle import pyoracle as po
from test_gpu_device_streams import delay  # noqa: F401  (the calibrated GPU delay that makes a caller's stream busy)
from vgaudio_amd import _lib
from vgaudio_amd import adx
from vgaudio_amd.adx import AdxFileSet
from vgaudio_amd.criadx import CriAdxKey
from vgaudio_amd.gcadpcm import Pcm16Format

pytestmark = pytest.mark.gpu

# function of the header -> the tests below that call it
CASES = {
    "vga_adx_write_keyed_device_v": [
        "test_keyed_images_are_the_oracles_and_the_per_file_calls", "test_write_then_read_with_the_same_indices_returns_the_rows",
        "test_forced_general_form_gives_the_same_bytes", "test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream",
        "test_two_streams_at_once", "test_refused_calls_launch_nothing", "test_write_files_with_a_key_is_the_writers_get_file"],
    "vga_adx_read_keyed_device_v": [
        "test_keyed_rows_are_the_oracles_and_the_per_file_calls", "test_write_then_read_with_the_same_indices_returns_the_rows",
        "test_forced_general_form_gives_the_same_bytes", "test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream",
        "test_two_streams_at_once", "test_refused_calls_launch_nothing", "test_read_files_with_keys_is_the_readers_read_format"],
    "vga_adx_find_keys_workspace_bytes": ["test_found_keys_are_the_oracles_and_the_per_file_calls", "test_refused_calls_launch_nothing"],
    "vga_adx_find_keys_device_v": [
        "test_found_keys_are_the_oracles_and_the_per_file_calls", "test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream",
        "test_two_streams_at_once", "test_refused_calls_launch_nothing", "test_read_files_with_keys_is_the_readers_read_format"],
    "vga_adx_find_keys_items_for": ["test_found_keys_are_the_oracles_and_the_per_file_calls"],
}

JUNK = 0xEE
EXTRA = 64                                                             # junk in front of and behind every buffer (keeps 16-byte alignment)
POOL_STREAMS = 32                                                      # torch hands out this many streams, round robin


def torch():
    import torch as t
    return t


def L():
    return _lib.lib()


def dev(a):
    return torch().from_numpy(np.array(a, copy=True, order="C")).cuda()


def host(t):
    return t.cpu().numpy()


def stream_ptr(stream=None):
    return C.c_void_p((stream if stream is not None else torch().cuda.current_stream()).cuda_stream)


def d_keys(names):
    return dev(np.array([kc.KEYS[k] for k in names], np.int32).reshape(-1))


def ckey(name):
    return _lib.AdxKeyC(*kc.KEYS[name])


_expected = {}


def key_names(index_name):
    """the key every file is moved under with that set of indices (None: unkeyed), and the status the call writes"""
    index = kc.key_index_sets()[index_name]
    index = [0] * len(kc.FILES) if index is None else index
    return [kc.key_of_index(i) for i in index], [1 if i >= len(kc.ALL_KEYS) else 0 for i in index]


def expected_images(index_name):
    if index_name not in _expected:
        t, out = kc.table(), []
        for n, name in enumerate(key_names(index_name)[0]):
            if name == kc.FILES[n][2]:
                out.append(t["keyed"][n])
            elif name is None:
                out.append(t["plain"][n])
            else:
                out.append(kc.image_of(t["files"][n], t["rows"][n], t["hist"][n], name))
        _expected[index_name] = out
    return _expected[index_name]


def expected_rows(index_name):
    """what the keyed read leaves of the table's keyed images under those indices"""
    key = ("rows", index_name)
    if key not in _expected:
        t, out = kc.table(), []
        for n, name in enumerate(key_names(index_name)[0]):
            info = t["infos"][n]
            if name == kc.FILES[n][2]:
                out.append(t["dec_rows"][n])
            else:
                out.append(kc.crypt(t["enc_rows"][n], name, info.revision, info.frame_size))
        _expected[key] = out
    return _expected[key]


def d_index(index_name):
    index = kc.key_index_sets()[index_name]
    return None if index is None else dev(np.array(index, np.int32))


class WriteSet:
    def __init__(self, offsets_name="packed"):
        t = kc.table()
        self.files, self.rows = t["files"], [r for rows in t["rows"] for r in rows]
        self.hist = np.concatenate(t["hist"]).astype(np.int16)
        self.offs = None if offsets_name == "packed" else ac.explicit_offsets(self.files, 4)
        self.s = AdxFileSet(self.files, self.offs)
        self.keys = d_keys(kc.ALL_KEYS)

    def close(self):
        self.s.close()

    def audio(self, fill=JUNK):
        a = np.full(self.s.totals.audio_bytes, fill, np.uint8)
        for c, row in enumerate(self.rows):
            a[self.s.audio_offsets[c]:self.s.audio_offsets[c] + len(row)] = row
        return dev(a)

    def images(self, fill=JUNK):
        return torch().full((self.s.totals.image_bytes + 2 * EXTRA,), fill, dtype=torch().uint8, device="cuda")

    def status(self):
        return torch().full((len(self.files) + 8,), 0x5555, dtype=torch().int32, device="cuda")

    def run(self, audio, images, index_name, stream=None, history=None, status=None):
        history = history if history is not None else dev(self.hist)
        index = d_index(index_name)
        self.keep = (history, index)
        _lib.check(L().vga_adx_write_keyed_device_v(self.s._h, audio.data_ptr(), history.data_ptr(), self.keys.data_ptr(), len(kc.ALL_KEYS),
                                                    index.data_ptr() if index is not None else None, images.data_ptr() + EXTRA,
                                                    status.data_ptr() if status is not None else None, stream_ptr(stream)))
        return images

    def check(self, images, index_name, what, fill=JUNK):
        """every image is the oracle's, every other byte of the buffer is what it was"""
        got = host(images).copy()
        assert np.all(got[:EXTRA] == fill) and np.all(got[-EXTRA:] == fill), (what, "outside the buffer")
        got = got[EXTRA:-EXTRA]
        for f, (at, want) in enumerate(zip(self.s.image_offsets, expected_images(index_name))):
            mine = got[at:at + len(want)]
            if not np.array_equal(mine, want):
                bad = np.flatnonzero(mine != want)
                raise AssertionError((what, "file", f, kc.FILES[f], "first bad byte", int(bad[0]), "of", len(want), "bad bytes", len(bad)))
            got[at:at + len(want)] = fill
        assert np.all(got == fill), (what, "bytes outside the images were written", np.flatnonzero(got != fill)[:8])


def check_status(status, index_name):
    h = host(status)
    want = key_names(index_name)[1]
    assert list(h[:len(want)]) == want and np.all(h[len(want):] == 0x5555), index_name


# ---------------------------------------------------------------- 1. write
@pytest.mark.parametrize("offsets,index_name", [("packed", "own"), ("packed", "null"), ("explicit4", "mixed")])
def test_keyed_images_are_the_oracles_and_the_per_file_calls(offsets, index_name):
    t = torch()
    a = WriteSet(offsets)
    try:
        audio, status = a.audio(), a.status()
        before = audio.clone()
        images = a.run(audio, a.images(), index_name, status=status)
        t.cuda.synchronize()
        a.check(images, index_name, (offsets, index_name))
        check_status(status, index_name)
        assert t.equal(audio, before), "d_audio was changed"
        # vga_adx_crypt_device on a copy of every file's rows, then vga_adx_write_device
        at, want = 0, expected_images(index_name)
        for f, (file, name) in enumerate(zip(a.files, key_names(index_name)[0])):
            n, nch = ac.row_bytes(file), file.channels
            pitch = ac.up(max(n, 1), 16)
            staged = np.full((nch, pitch), JUNK, np.uint8)
            for c in range(nch):
                staged[c, :n] = a.rows[at + c]
            d_rows, d_hist = dev(staged), dev(a.hist[at:at + nch])
            if name is not None:
                _lib.check(L().vga_adx_crypt_device(d_rows.data_ptr(), pitch, n, nch, C.byref(ckey(name)), file.params.encryption_type,
                                                    file.params.frame_size, stream_ptr()))
            d_file = t.full((len(want[f]) + 32,), JUNK, dtype=t.uint8, device="cuda")
            _lib.check(L().vga_adx_write_device(d_rows.data_ptr(), pitch, n, d_hist.data_ptr(), nch, C.byref(file.params), d_file.data_ptr(), stream_ptr()))
            assert np.array_equal(host(d_file)[:len(want[f])], want[f]), ("per-file calls", f, kc.FILES[f])
            at += nch
    finally:
        a.close()


# ---------------------------------------------------------------- 2. read
def pack_images(images, offsets, total, fill=JUNK):
    packed = np.full(total + 2 * 16, fill, np.uint8)                     # (the set's own guard lies behind the last image)
    for image, at in zip(images, offsets):
        packed[at:at + len(image)] = image
    return packed[:total]


class ReadSet:
    """the table's keyed images (each under its own key), as the reader sees them: up to the end of the audio"""

    def __init__(self, offsets_name="packed", fill=JUNK):
        t = kc.table()
        self.infos = t["infos"]
        self.sizes = [i.audio_offset + i.audio_bytes * i.channel_count for i in self.infos]
        self.offs = ac.odd_image_offsets(self.sizes) if offsets_name == "odd" else None
        self.s = AdxFileSet.from_infos(self.infos, self.offs)
        self.packed = pack_images([w[:n] for w, n in zip(t["keyed"], self.sizes)], self.s.image_offsets, self.s.totals.image_bytes, fill)
        self.keys = d_keys(kc.ALL_KEYS)

    def close(self):
        self.s.close()

    def rows(self, fill=JUNK):
        return torch().full((self.s.totals.audio_bytes,), fill, dtype=torch().uint8, device="cuda")

    def run(self, d_images, rows, index, stream=None, history=None, status=None, keys=None, nkeys=None):
        keys = keys if keys is not None else self.keys
        _lib.check(L().vga_adx_read_keyed_device_v(self.s._h, d_images.data_ptr(), keys.data_ptr(), nkeys or keys.numel() // 3,
                                                   index.data_ptr() if index is not None else None, rows.data_ptr(),
                                                   history.data_ptr() if history is not None else None,
                                                   status.data_ptr() if status is not None else None, stream_ptr(stream)))
        return rows

    def check(self, got, want_rows, what, fill=JUNK):
        got, c = got.copy(), 0
        for f, info in enumerate(self.infos):
            for ch in range(info.channel_count):
                n, at = info.audio_bytes, int(self.s.audio_offsets[c])
                if not np.array_equal(got[at:at + n], want_rows[f][ch][:n]):
                    bad = np.flatnonzero(got[at:at + n] != want_rows[f][ch][:n])
                    raise AssertionError((what, "file", f, kc.FILES[f], "channel", ch, "first bad byte", int(bad[0]), "bad bytes", len(bad)))
                got[at:at + n] = fill
                c += 1
        assert np.all(got == fill), (what, "bytes outside the rows were written", np.flatnonzero(got != fill)[:8])


@pytest.mark.parametrize("offsets,index_name", [("packed", "own"), ("odd", "mixed"), ("odd", "null")])
def test_keyed_rows_are_the_oracles_and_the_per_file_calls(offsets, index_name):
    t = torch()
    r = ReadSet(offsets)
    try:
        assert r.offs is None or list(r.s.image_offsets) == r.offs
        d_images, index = dev(r.packed), d_index(index_name)
        hist = t.full((r.s.channels + 8,), 0x7777, dtype=t.int16, device="cuda")
        status = t.full((len(r.infos) + 8,), 0x5555, dtype=t.int32, device="cuda")
        rows = r.run(d_images, r.rows(), index, history=hist, status=status)
        t.cuda.synchronize()
        want = expected_rows(index_name)
        r.check(host(rows), want, (offsets, index_name))
        check_status(status, index_name)
        h = host(hist)
        assert list(h[:r.s.channels]) == [int(i.history[c][0]) for i in r.infos for c in range(i.channel_count)] and np.all(h[r.s.channels:] == 0x7777)
        assert np.array_equal(host(d_images), r.packed), "d_images was changed"
        # vga_adx_read_device, then vga_adx_crypt_device with encryption_type = revision, for every file alone
        keyed = kc.table()["keyed"]
        for f, (info, name) in enumerate(zip(r.infos, key_names(index_name)[0])):
            if info.audio_bytes == 0:
                continue
            pitch = ac.up(info.audio_bytes, 16)
            d_file = dev(keyed[f][:r.sizes[f]])
            out = t.full((info.channel_count, pitch), JUNK, dtype=t.uint8, device="cuda")
            _lib.check(L().vga_adx_read_device(C.byref(info), d_file.data_ptr(), r.sizes[f], 1, out.data_ptr(), pitch, stream_ptr()))
            if name is not None:
                _lib.check(L().vga_adx_crypt_device(out.data_ptr(), pitch, info.audio_bytes, info.channel_count, C.byref(ckey(name)), info.revision,
                                                    info.frame_size, stream_ptr()))
            got = host(out)
            for ch in range(info.channel_count):
                assert np.array_equal(got[ch, :info.audio_bytes], want[f][ch][:info.audio_bytes]), ("per-file calls", f, ch)
    finally:
        r.close()


def test_write_then_read_with_the_same_indices_returns_the_rows():
    """keyed write, a set from the parsed headers over the SAME buffer, keyed read with the same index array: the input rows for
    types 8, 0 and 5, the rows with every non-empty frame's first byte masked for type 9 -- up to what the file kept"""
    t = torch()
    a = WriteSet("packed")
    try:
        images = a.run(a.audio(), a.images(), "mixed")
        index = a.keep[1]
        infos = kc.table()["infos"]                                    # (a key changes no header: the table's infos are these images')
        r = AdxFileSet.from_infos(infos, [int(o) for o in a.s.image_offsets])
        try:
            rows = t.full((r.totals.audio_bytes,), JUNK, dtype=t.uint8, device="cuda")
            assert r.totals.image_bytes <= a.s.totals.image_bytes
            view = images[EXTRA:EXTRA + r.totals.image_bytes]
            _lib.check(L().vga_adx_read_keyed_device_v(r._h, view.data_ptr(), a.keys.data_ptr(), len(kc.ALL_KEYS), index.data_ptr(), rows.data_ptr(),
                                                       None, None, stream_ptr()))
            t.cuda.synchronize()
            got, c, masked = host(rows), 0, 0
            for f, (file, info) in enumerate(zip(a.files, infos)):
                keep = min(info.audio_bytes, ac.row_bytes(file))
                keyed = key_names("mixed")[0][f] is not None
                for ch in range(file.channels):
                    at, want = int(r.audio_offsets[c]), np.array(a.rows[c][:keep], copy=True)
                    if keyed and info.revision == 9:
                        frames = want.reshape(-1, info.frame_size)
                        frames[frames.any(axis=1), 0] &= 0x1F
                        masked += 1
                    assert np.array_equal(got[at:at + keep], want), (f, ch, kc.FILES[f])
                    c += 1
            assert masked
        finally:
            r.close()
    finally:
        a.close()


# ---------------------------------------------------------------- 3. the search
def run_find(r, d_images, name, workspace, stream=None):
    k8, k9 = kc.FIND_LISTS[name]
    keys = d_keys(k8 + k9) if k8 or k9 else None
    out = torch().full((len(r.infos) + 8,), 0x5555, dtype=torch().int32, device="cuda")
    need = L().vga_adx_find_keys_workspace_bytes(r.s._h, len(k8), len(k9))
    assert need == kc.workspace_model(len(r.infos), len(k8), len(k9)) and workspace.numel() >= need
    _lib.check(L().vga_adx_find_keys_device_v(r.s._h, d_images.data_ptr(), keys.data_ptr() if keys is not None else None, len(k8), len(k9),
                                              out.data_ptr(), workspace.data_ptr(), need, stream_ptr(stream)))
    return out, keys


@pytest.mark.parametrize("fill", [0xFF, 0x00])
@pytest.mark.parametrize("offsets,name", [("packed", "forward"), ("odd", "reverse"), ("packed", "absent"), ("odd", "empty9")])
def test_found_keys_are_the_oracles_and_the_per_file_calls(offsets, name, fill):
    t = torch()
    r = ReadSet(offsets)
    try:
        items = AdxFileSet.find_items(r.infos, r.offs)
        assert [(i.file, i.first_slot, i.slot_count) for i in items] == kc.find_items_model(r.infos)
        d_images = dev(r.packed)
        workspace = t.full((kc.workspace_model(len(r.infos), 6, 3) + 64,), fill, dtype=t.uint8, device="cuda")
        want = kc.table()["found"][name]
        for again in range(2):                                         # the second run finds the workspace as the first one left it
            out, keys = run_find(r, d_images, name, workspace)
            t.cuda.synchronize()
            h = host(out)
            assert list(h[:len(want)]) == want and np.all(h[len(want):] == 0x5555), (name, again, [(n, int(g), w) for n, (g, w) in enumerate(zip(h, want)) if g != w])
        assert np.all(host(workspace)[-64:] == fill), "bytes behind the workspace's size were written"
        assert np.array_equal(host(d_images), r.packed)
        if fill == 0xFF:                                               # vga_adx_find_key_device over the sub-list, for every file alone
            k8, k9 = kc.FIND_LISTS[name]
            enc = kc.table()["enc_rows"]
            for f, info in enumerate(r.infos):
                sub, base = (k8, 0) if info.revision == 8 else (k9, len(k8))
                if info.revision == 0 or not sub:
                    assert want[f] == -1
                    continue
                pitch = ac.up(max(info.audio_bytes, 1), 16)
                staged = np.full((info.channel_count, pitch), JUNK, np.uint8)
                for c in range(info.channel_count):
                    staged[c, :info.audio_bytes] = enc[f][c]
                d_rows, arr, idx = dev(staged), (_lib.AdxKeyC * len(sub))(*[ckey(k) for k in sub]), C.c_int(-7)
                _lib.check(L().vga_adx_find_key_device(d_rows.data_ptr(), pitch, info.audio_bytes, info.channel_count, info.revision, info.frame_size,
                                                       arr, len(sub), C.byref(idx), stream_ptr()))
                assert (idx.value + base if idx.value >= 0 else -1) == want[f], ("per-file call", f, kc.FILES[f])
    finally:
        r.close()


# ---------------------------------------------------------------- 4. forms
def test_forced_general_form_gives_the_same_bytes():
    t = torch()
    a, r = WriteSet("packed"), ReadSet("packed")
    try:
        mixed_w, mixed_r = a.s.stats(), r.s.stats()
        assert min(mixed_w) > 0 and min(mixed_r) > 0, (mixed_w, mixed_r)
        d_images, index = dev(r.packed), d_index("own")
        assert L().vga_adx_files_force_general_this_thread(1) == 0
        try:
            forced_w, forced_r = a.s.stats(), r.s.stats()
            assert forced_w[0] == forced_w[2] == 0 and forced_r[0] == forced_r[2] == 0
            images = a.run(a.audio(), a.images(), "own")
            rows = r.run(d_images, r.rows(), index)
            t.cuda.synchronize()
        finally:
            assert L().vga_adx_files_force_general_this_thread(0) == 1
        a.check(images, "own", "forced general")
        r.check(host(rows), expected_rows("own"), "forced general")
        again = a.run(a.audio(), a.images(), "own")
        t.cuda.synchronize()
        assert t.equal(again, images)
    finally:
        r.close()
        a.close()


# ---------------------------------------------------------------- 5. poison mode
@pytest.mark.parametrize("value", [0xA5, 0xFF])
def test_bytes_do_not_depend_on_poison(value):
    t = torch()
    old = L().vga_testing_poison_allocations(value)
    fill = value ^ 0x3C
    try:
        a = WriteSet("packed")                                         # (created under the mode: its tables are poisoned first)
        try:
            images = a.run(a.audio(fill), a.images(fill), "mixed")
            t.cuda.synchronize()
            a.check(images, "mixed", ("poison", value), fill=fill)
        finally:
            a.close()
        r = ReadSet("packed", fill=value)
        try:
            d_images = dev(r.packed)
            rows = r.run(d_images, r.rows(fill), d_index("mixed"))
            workspace = t.full((kc.workspace_model(len(r.infos), 6, 3),), value, dtype=t.uint8, device="cuda")
            out, keys = run_find(r, d_images, "forward", workspace)
            t.cuda.synchronize()
            r.check(host(rows), expected_rows("mixed"), ("poison", value), fill=fill)
            assert list(host(out)[:len(r.infos)]) == kc.table()["found"]["forward"]
        finally:
            r.close()
    finally:
        t.cuda.synchronize()
        L().vga_testing_poison_allocations(old if old >= 0 else -1)


# ---------------------------------------------------------------- 6. streams
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


def test_calls_on_a_busy_stream(delay):  # noqa: F811
    """The keyed write, and the chain search -> keyed read with the search's index tensor, queued behind a delay on the caller's
    stream: they do not wait for it and nothing reads the indices on the host; they are ordered after the delay -- their
    inputs are written on the same stream behind it"""
    t = torch()
    cycles, ms = delay
    a, r = WriteSet("packed"), ReadSet("packed")
    try:
        (S,) = some_streams(1)
        source, d_packed, d_hist = a.audio(), dev(r.packed), dev(a.hist)
        k8, k9 = kc.FIND_LISTS["reverse"]
        keys = d_keys(k8 + k9)
        workspace = t.full((kc.workspace_model(len(r.infos), len(k8), len(k9)),), 0x77, dtype=t.uint8, device="cuda")
        with t.cuda.stream(S):
            for busy in (False, True):                                 # (warm first: every kernel has run once)
                d_audio, d_images = t.zeros_like(source), t.zeros_like(d_packed)
                images, rows = a.images(), r.rows()
                S.synchronize()
                if busy:
                    t.cuda._sleep(cycles)
                d_audio.copy_(source, non_blocking=True)               # the inputs arrive behind the delay
                d_images.copy_(d_packed, non_blocking=True)
                a.run(d_audio, images, "own", stream=S, history=d_hist)
                found, _ = run_find(r, d_images, "reverse", workspace, stream=S)
                r.run(d_images, rows, found, stream=S, keys=keys)
                if busy:
                    assert not S.query(), "the caller's stream was idle when the calls returned (they waited for it)"
        S.synchronize()
        a.check(images, "own", "busy stream")
        # the rows under the keys the search named: decrypted where it found the file's key, as they were where it found none
        want_found = kc.table()["found"]["reverse"]
        assert list(host(found)[:len(r.infos)]) == want_found
        t_ = kc.table()
        want = [kc.crypt(t_["enc_rows"][f], (k8 + k9)[i] if i >= 0 else None, info.revision, info.frame_size)
                for f, (i, info) in enumerate(zip(want_found, r.infos))]
        r.check(host(rows), want, "busy stream")
        assert sum(i >= 0 for i in want_found) > 0
    finally:
        r.close()
        a.close()


def test_two_streams_at_once():
    """one object for each direction, two streams each"""
    t = torch()
    a, r = WriteSet("explicit4"), ReadSet("odd")
    try:
        S1, S2 = some_streams(2)
        d_audio, i1, i2, d_hist = a.audio(), a.images(), a.images(0x11), dev(a.hist)
        d_images, index = dev(r.packed), d_index("own")
        r1, r2 = r.rows(JUNK), r.rows(0x11)
        w1, w2 = (t.full((kc.workspace_model(len(r.infos), 6, 3),), v, dtype=t.uint8, device="cuda") for v in (0, 0xFF))
        t.cuda.synchronize()
        a.run(d_audio, i1, "own", stream=S1, history=d_hist)
        a.run(d_audio, i2, "own", stream=S2, history=d_hist)
        r.run(d_images, r1, index, stream=S1)
        r.run(d_images, r2, index, stream=S2)
        f1, k1 = run_find(r, d_images, "forward", w1, stream=S1)
        f2, k2 = run_find(r, d_images, "forward", w2, stream=S2)
        S1.synchronize()
        S2.synchronize()
        a.check(i1, "own", "stream 1")
        a.check(i2, "own", "stream 2", fill=0x11)
        r.check(host(r1), expected_rows("own"), "stream 1")
        r.check(host(r2), expected_rows("own"), "stream 2", fill=0x11)
        want = kc.table()["found"]["forward"]
        assert list(host(f1)[:len(want)]) == want and list(host(f2)[:len(want)]) == want
    finally:
        r.close()
        a.close()


# ---------------------------------------------------------------- 7. refused calls
def test_refused_calls_launch_nothing():
    t = torch()
    a, r = WriteSet("packed"), ReadSet("packed")
    try:
        d_audio, images, d_hist = a.audio(), a.images(), dev(a.hist)
        rows, d_images, keys, n = r.rows(), dev(r.packed), a.keys.data_ptr(), len(kc.ALL_KEYS)
        out = t.full((len(r.infos),), 0x5555, dtype=t.int32, device="cuda")
        status = t.full((len(r.infos),), 0x5555, dtype=t.int32, device="cuda")
        need = L().vga_adx_find_keys_workspace_bytes(r.s._h, 6, 3)
        assert need == kc.workspace_model(len(r.infos), 6, 3) and L().vga_adx_find_keys_workspace_bytes(a.s._h, 6, 3) == 0
        workspace = t.full((need,), JUNK, dtype=t.uint8, device="cuda")
        w, rd, fd = L().vga_adx_write_keyed_device_v, L().vga_adx_read_keyed_device_v, L().vga_adx_find_keys_device_v
        st, base, sp = stream_ptr(), images.data_ptr() + EXTRA, status.data_ptr()
        A, H, R, I, O, W = d_audio.data_ptr(), d_hist.data_ptr(), rows.data_ptr(), d_images.data_ptr(), out.data_ptr(), workspace.data_ptr()
        assert rd(a.s._h, base, keys, n, None, A, None, sp, st) == -4      # a set for writing refuses the read and find calls
        assert fd(a.s._h, base, keys, 6, 3, O, W, need, st) == -4
        assert w(r.s._h, R, H, keys, n, None, base, sp, st) == -4          # ... and the other way round
        assert w(a.s._h, A, H, None, n, None, base, sp, st) == -1          # keys
        assert w(a.s._h, A, H, keys, 0, None, base, sp, st) == -1
        assert w(a.s._h, A, H, keys, -1, None, base, sp, st) == -1
        assert w(a.s._h, A, None, keys, n, None, base, sp, st) == -1       # adx_files.h's checks
        assert w(a.s._h, None, H, keys, n, None, base, sp, st) == -1
        assert w(a.s._h, A, H, keys, n, None, None, sp, st) == -1
        assert w(a.s._h, A + 4, H, keys, n, None, base, sp, st) == -1
        assert w(a.s._h, A, H, keys, n, None, base + 8, sp, st) == -1
        assert rd(r.s._h, I, None, n, None, R, None, sp, st) == -1
        assert rd(r.s._h, I, keys, 0, None, R, None, sp, st) == -1
        assert rd(r.s._h, I + 1, keys, n, None, R, None, sp, st) == -1
        assert rd(r.s._h, I, keys, n, None, R + 2, None, sp, st) == -1
        assert rd(r.s._h, None, keys, n, None, R, None, sp, st) == -1
        assert fd(r.s._h, I, None, 6, 3, O, W, need, st) == -1
        assert fd(r.s._h, I, keys, -1, 3, O, W, need, st) == -1
        assert fd(r.s._h, I, keys, 6, -3, O, W, need, st) == -1
        assert fd(r.s._h, I, keys, 6, 3, None, W, need, st) == -1
        assert fd(r.s._h, I, keys, 6, 3, O, None, need, st) == -1
        assert fd(r.s._h, I, keys, 6, 3, O, W, need - 1, st) == -1
        assert fd(r.s._h, I + 1, keys, 6, 3, O, W, need, st) == -1
        t.cuda.synchronize()
        assert np.all(host(images) == JUNK) and np.all(host(rows) == JUNK) and np.all(host(workspace) == JUNK)
        assert np.all(host(out) == 0x5555) and np.all(host(status) == 0x5555)
    finally:
        r.close()
        a.close()


# ---------------------------------------------------------------- 8. the Python layer
def lead_in_files():
    """seeded PCM with a silent lead-in (all-zero frames in front, as encrypted game audio has): mono and stereo, looping and not"""
    rng = np.random.default_rng(0x5EED8)
    out = []
    for nch, n, rate, loop, lead in ((1, 3000, 48000, None, 640), (2, 2777, 44100, (5, 2700), 320), (2, 640, 48000, None, 0),
                                     (1, 1500, 32000, (33, 1480), 96), (2, 4000, 44100, None, 2048)):
        chans = []
        for _ in range(nch):
            pcm = (rng.integers(-3000, 3000, n) * np.linspace(0.2, 1.0, n)).astype(np.int16)
            pcm[:lead] = 0
            chans.append(pcm)
        f = Pcm16Format(chans, rate)
        if loop:
            f.Looping, f.LoopStart, f.LoopEnd = True, loop[0], loop[1]
        out.append(f)
    return out


def same_format(a, b, what):
    assert (a.ChannelCount, a.SampleRate, a.Looping, a.SampleCount, a.AlignmentSamples) == (b.ChannelCount, b.SampleRate, b.Looping, b.SampleCount, b.AlignmentSamples), what
    assert (a.LoopStart, a.LoopEnd, a.UnalignedSampleCount) == (b.LoopStart, b.LoopEnd, b.UnalignedSampleCount), what
    for c, (x, y) in enumerate(zip(a.Channels, b.Channels)):
        assert np.array_equal(np.asarray(x.Audio), np.asarray(y.Audio)) and x.History == y.History, (what, c)


@pytest.mark.parametrize("etype", [8, 9])
def test_write_files_with_a_key_is_the_writers_get_file(etype):
    files = lead_in_files()
    key = CriAdxKey(*kc.KEYS["high_seed" if etype == 8 else "nine_a"])
    config = adx.AdxConfiguration(EncryptionKey=key, EncryptionType=etype)
    got = adx.write_files(files, config)
    assert len(got) == len(files)
    plain = adx.write_files(files, adx.AdxConfiguration(EncryptionType=etype))
    for k, f in enumerate(files):
        assert got[k] == adx.AdxWriter(config).GetFile(f), ("file", k)
        assert got[k] != plain[k] and len(got[k]) == len(plain[k])


@pytest.mark.parametrize("etype", [8, 9])
def test_read_files_with_keys_is_the_readers_read_format(etype):
    files = lead_in_files()
    names = ["plain", "even_mult"] if etype == 8 else ["nine_a", "nine_b"]
    right, other, stranger = CriAdxKey(*kc.KEYS[names[0]]), CriAdxKey(*kc.KEYS[names[1]]), CriAdxKey(0x1357, 0x2469, 0x0ACF)
    images = [adx.AdxWriter(adx.AdxConfiguration(EncryptionKey=right, EncryptionType=etype)).GetFile(f) for f in files[:-1]]
    images.append(adx.AdxWriter(adx.AdxConfiguration(EncryptionKey=stranger, EncryptionType=etype)).GetFile(files[-1]))   # no candidate fits
    images.append(adx.AdxWriter(adx.AdxConfiguration()).GetFile(files[0]))                                               # not encrypted
    # a given key is applied to every file
    for k, (image, fmt) in enumerate(zip(images, adx.read_files(images, EncryptionKey=right))):
        same_format(fmt, adx.AdxReader(EncryptionKey=right).ReadFormat(image), ("key", k))
    # the key of every file is searched among the candidates
    keys = [other, right]
    got = adx.read_files(images, Keys=keys)
    untouched = adx.read_files(images)
    for k, (image, fmt) in enumerate(zip(images, got)):
        same_format(fmt, adx.AdxReader(Keys=keys).ReadFormat(image), ("keys", k))
    same_format(got[-2], untouched[-2], "no candidate fits: the audio stays encrypted")
    same_format(got[-1], untouched[-1], "revision 0 is not searched")
    assert not np.array_equal(np.asarray(got[0].Channels[0].Audio), np.asarray(untouched[0].Channels[0].Audio))
    split = adx.read_files(images, Keys8=keys if etype == 8 else [], Keys9=keys if etype == 9 else [])
    for k, (x, y) in enumerate(zip(split, got)):
        same_format(x, y, ("split lists", k))
    # the oracle's reader and cipher on the first file
    rc, h, hist, chans = po.adxfile_read(images[0])
    assert rc == 0
    want = po.adx_crypt([c[:got[0].Channels[0].Audio.size] for c in chans], po.AdxKey(*kc.KEYS[names[0]]), etype, 18)
    for c in range(h.channel_count):
        assert np.array_equal(np.asarray(got[0].Channels[c].Audio), want[c])

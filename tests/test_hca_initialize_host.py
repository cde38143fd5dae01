"""vga_hca_encoder_initialize (CriHcaEncoder.Initialize, CriHcaEncoder.cs:61-114) against the oracle's, every field of
HcaInfo, over the table of tests/hca_init_cases.py.  Host code: no GPU.  Where both refuse, the library's code and
message are the ones recorded in that table."""
import ctypes as C

import pytest

import hca_init_cases as T
from oracle import pyoracle as po
from oracle.pyref import crihca as pyref
from vgaudio_amd import _lib

CASES = T.cases()


def library_init(p):
    """(rc, HcaInfoC, message)"""
    cp, h = _lib.HcaParamsC(*p), _lib.HcaInfoC()
    rc = _lib.lib().vga_hca_encoder_initialize(C.byref(cp), C.byref(h))
    return rc, h, _lib.lib().vga_last_error().decode() if rc else ""


def oracle_init(p):
    """(refused, HcaInfo).  A looping stream with FrameSize 0 makes the reference divide by zero (CalculateHeaderSize :411,
    DivideByZeroException) and the C oracle with it, which C cannot catch: such a case is not handed to it (pyref throws
    there, test_the_reference_divides_by_zero_for_a_looping_frame_size_of_0)."""
    if p[6]:
        plain = po.HcaParams(*p)
        plain.looping = 0
        rc, info = po.hca_init(plain)                       # FrameSize does not depend on the loop
        if rc == 0 and info.frame_size == 0:
            return True, None
    rc, info = po.hca_init(po.HcaParams(*p))
    return rc != 0, info


def test_the_table_covers_what_it_names():
    assert 300 <= len(CASES) <= 900
    ok = [library_init(p)[1] for p in CASES if p not in T.PARENT_REFUSALS]
    assert {h.channel_count for h in ok} == set(range(1, 9))
    assert any(h.frame_size == 0 for h in ok) and any(h.looping and h.frame_count * 1024 > h.sample_count + 3 * 1024 for h in ok)
    _, h, _ = library_init(T.PADDING_INSERTS_FRAMES)
    assert (h.frame_size, h.inserted_samples, h.header_size) == (682, 128 + 2 * 1024, 96 + 1952 % 682)
    _, h, _ = library_init(T.PADDING_INSERTS_NONE)
    assert (h.frame_size, h.inserted_samples, h.header_size) == (4096, 128, 96 + 1952)
    assert sum(1 for p in CASES if p in T.PARENT_REFUSALS) == len(T.PARENT_REFUSALS) - 1       # all but the negative count


def test_initialize_matches_the_oracle_field_by_field():
    for p in CASES:
        rc, h, msg = library_init(p)
        refused, want = oracle_init(p)
        assert (rc != 0) == refused, (p, rc, msg)
        if refused:
            assert (rc, msg) == T.PARENT_REFUSALS[p], p
            continue
        assert p not in T.PARENT_REFUSALS, p
        for name, _ in po.HcaInfo._fields_:
            assert getattr(h, name) == getattr(want, name), (p, name, getattr(h, name), getattr(want, name))


def test_the_reference_divides_by_zero_for_a_looping_frame_size_of_0():
    quality, bitrate, limit, nch, rate, n, _, start, end = T.LOOPING_FRAME_SIZE_0
    with pytest.raises(ZeroDivisionError):
        pyref.Encoder(pyref.Params(nch, rate, n, quality=quality, bitrate=bitrate, limit_bitrate=bool(limit), looping=True,
                                   loop_start=start, loop_end=end))
    assert oracle_init(T.LOOPING_FRAME_SIZE_0) == (True, None)
    assert library_init(T.LOOPING_FRAME_SIZE_0)[0] == _lib.VGA_ERR_INVALID_DATA


def test_a_negative_sample_count_is_refused():
    """the library's own check: the reference and the oracle take a negative SampleCount (not compared with them)"""
    rc, _, msg = library_init(T.NEGATIVE_COUNT)
    assert (rc, msg) == T.PARENT_REFUSALS[T.NEGATIVE_COUNT]
    assert _lib.lib().vga_hca_encoder_initialize(None, None) == _lib.VGA_ERR_ARGUMENT
    assert _lib.lib().vga_last_error().decode() == "null argument"

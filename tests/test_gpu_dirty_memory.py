"""Every entry point on dirty memory (include/vgaudio_hip_testing.h: vga_testing_poison_allocations).

The device pool hands a parked block to any later request of half its size or more with the last call's bytes in it, the
page-locked pool any idle block that is large enough, and the runtime recycles stream-ordered scratch; the rest of the
suite allocates a few KB at a time and so only ever sees the zeros of fresh driver memory.  Here

  a. the host-pointer entry points run with every allocation of the library filled with 0xA5 and with 0xFF first: the 13
     batch cases of test_gpu_host_paths.CASES in both forced pipeline shapes, and the other host-pointer calls through
     the oracle-backed checks the suite already has (HOST_CHECKS);
  b. the device entry points run with poisoned scratch AND junk in every padding column of their input rows (the rows of
     test_gpu_device_streams.ROWS and test_gpu_pcm_device_streams.ROWS), and must leave every input byte as it was; the
     busy-stream tests run once more in poison mode;
  c. every function of the four headers is driven by (a) or (b) or listed in EXEMPT with a reason -- statically (CPU) and, on
     the GPU, by a recorder on the ctypes library that notes which functions were really called in poison mode;
  d. with the hook off, five families hand the pool's blocks (1 MiB and more) to each other over three calls each.

Everything is compared with the C oracle or the tests/*_ref.py restatements; no result is compared with another run of
the library alone."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_device_streams as ds
from test_abi_exports import _declared_symbols
from test_gpu_device_streams import delay  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON_BYTES = [0xA5, 0xFF]


def _lib():
    from vgaudio_amd import _lib as m
    return m


def _setting():
    """the hook's current value, read without changing it"""
    L = _lib().lib()
    old = L.vga_testing_poison_allocations(-1)
    L.vga_testing_poison_allocations(old)
    return old


@pytest.fixture(autouse=True)
def hook_is_off_around_every_test():
    assert _setting() == -1, "poison mode was on when the test began"
    yield
    left = _setting()
    _lib().lib().vga_testing_poison_allocations(-1)
    assert left == -1, "the test left poison mode on"


# ---------------------------------------------------------------- the recorder: which library functions ran in poison mode
CALLED = set()                  # every function fetched from the library inside poisoned()
RAN = set()                     # the drivers of (a) and (b) that have run in this process


class _Recorder:
    """stands in for the ctypes library: notes the name of every function a caller fetches"""

    def __init__(self, real):
        object.__setattr__(self, "_real", real)

    def __getattr__(self, name):
        CALLED.add(name)
        return getattr(self._real, name)


@contextlib.contextmanager
def poisoned(byte):
    m = _lib()
    real = m.lib()
    assert not isinstance(real, _Recorder)
    assert real.vga_testing_poison_allocations(byte) == -1
    m._lib = _Recorder(real)
    try:
        yield
    finally:
        m._lib = real
        real.vga_testing_poison_allocations(-1)


# ---------------------------------------------------------------- CPU: the hook is host state
def test_hook_is_off_by_default_returns_the_previous_value_and_needs_no_device():
    """in a process of its own, with every GPU hidden from it"""
    code = ("from vgaudio_amd import _lib\n"
            "L = _lib.lib()\n"
            "f = L.vga_testing_poison_allocations\n"
            "assert f(0xA5) == -1\n"            # off by default
            "assert f(0xFF) == 0xA5\n"
            "assert f(0) == 0xFF\n"
            "assert f(256) == 0 and f(-2) == 0\n"   # out of range: unchanged
            "assert f(-1) == 0\n"
            "assert f(-1) == -1\n"
            "print('ok')\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ---------------------------------------------------------------- a. host-pointer entry points
# the entry point behind every case of test_gpu_host_paths.CASES
BATCH_CASES = {
    "gc_encode_batch": "vga_gcadpcm_encode_batch", "gc_decode_batch": "vga_gcadpcm_decode_batch",
    "gc_encode_batch_v": "vga_gcadpcm_encode_batch_v", "gc_coefs_batch_v": "vga_gcadpcm_calculate_coefficients_batch_v",
    "gc_decode_batch_v": "vga_gcadpcm_decode_batch_v", "adx_encode_batch": "vga_adx_encode_batch",
    "adx_decode_batch": "vga_adx_decode_batch", "adx_encode_batch_v": "vga_adx_encode_batch_v",
    "adx_decode_batch_v": "vga_adx_decode_batch_v", "hca_encode_batch": "vga_hca_encode_batch",
    "hca_decode_batch": "vga_hca_decode_batch", "hca_encode_batch_v": "vga_hca_encode_batch_v",
    "hca_decode_batch_v": "vga_hca_decode_batch_v",
}


def _host_checks():
    """name -> (module, function, arguments): oracle-backed checks the suite already has, one size each"""
    import nwstm_pcm_ref
    import nwwav_ref
    from vgaudio_amd.criadx import CriAdxType
    from vgaudio_amd.nwstm import NwTarget
    brstm, bcstm, bfstm = list(NwTarget)[:3]
    return {
        "dsp_file": ("test_gpu_dsp", "test_file_matches_oracle_geometries", (7, 50001, 14 * 1000)),
        "dsp_looping_file": ("test_gpu_dsp", "test_looping_files_match_oracle", (2, (1399, 9001), 0, False)),
        "dsp_round_trip": ("test_gpu_container_readers", "test_dsp_round_trip", (2, 30000, True)),
        "adx_file": ("test_gpu_containers", "test_adx_file_matches_oracle", (6, 20001, 4)),
        "adx_round_trip": ("test_gpu_container_readers", "test_adx_round_trip", (3, 20000, True, 3, CriAdxType.Exponential)),
        "adx_encrypted_files": ("test_gpu_container_readers", "test_adx_encrypted_files", (8,)),
        "hca_file": ("test_gpu_containers", "test_hca_file_matches_oracle", (2, 20000, (3000, 17000))),
        "hca_round_trip": ("test_gpu_container_readers", "test_hca_round_trip", (2, 100000, True)),
        "hca_encrypted_files": ("test_gpu_container_readers", "test_hca_encrypted_files", ()),
        "brstm_gc": ("test_gpu_nwstm", "test_geometry_grid", (brstm, 1)),
        "bcstm_gc": ("test_gpu_nwstm", "test_geometry_grid", (bcstm, 3)),
        "bfstm_gc": ("test_gpu_nwstm", "test_geometry_grid", (bfstm, 2)),
        "brstm_pcm16": ("test_gpu_nwstm_pcm", "test_build_and_parse_equal", ("Brstm", nwstm_pcm_ref.PCM16, 2)),
        "bcstm_pcm8": ("test_gpu_nwstm_pcm", "test_build_and_parse_equal", ("Bcstm", nwstm_pcm_ref.PCM8, 8)),
        "bfstm_pcm8": ("test_gpu_nwstm_pcm", "test_build_and_parse_equal", ("Bfstm", nwstm_pcm_ref.PCM8, 1)),
        "hps": ("test_gpu_gc_containers", "test_hps_build_and_parse_equal", (2,)),
        "hps_unaligned_loop": ("test_gpu_gc_containers", "test_hps_unaligned_loop_from_pcm_uses_the_unaligned_decode", (2,)),
        "idsp": ("test_gpu_gc_containers", "test_idsp_images_equal_restatement", (3, 0x38, True, (1234, 40000))),
        "genh": ("test_gpu_gc_containers", "test_genh_reads_audio_and_coefficients", (2, 1, True, 19950)),
        "wave16": ("test_gpu_wave", "test_transposes_match_oracle", (33, 700)),
        "wave16_file": ("test_gpu_wave", "test_wave_pcm16_build_and_parse_equal", (2, True)),
        "wave8_file": ("test_gpu_wave_pcm8", "test_wave_pcm8_build_and_parse_equal", (2, True, 10001)),
        "nwwav_bank": ("test_gpu_nwwav", "test_bank_read_then_decode_against_the_oracle", ()),
        "nwwav_bank_rows": ("test_gpu_nwwav", "test_file_alignment_in_the_buffer", (16,)),
        "nwwav_prefetch_bank": ("test_gpu_nwwav", "test_bank_of_one_file", (nwwav_ref.FSTP, nwwav_ref.GCADPCM)),
        "gc_build_channels_loops": ("test_gpu_gcadpcm", "test_build_channels_matches_oracle", (20000, (2800, 2990), 0x3800, 0x3800)),
        "gc_build_channels_shift": ("test_gpu_gcadpcm", "test_build_channels_matches_oracle", (3000, (100, 2900), 1000, 0x200)),
        "gc_coefs": ("test_gpu_gcadpcm", "test_coefs_match_oracle_edge_inputs", (14 * 700 + 9,)),
        "gc_encode_with_coefs": ("test_gpu_gcadpcm", "test_encode_matches_oracle_edge_inputs_and_coefs", (14 * 300 + 3,)),
        "gc_ragged_with_coefs": ("test_gpu_ragged", "test_coefficients_only_and_encode_with_given_coefficients", ()),
        "adx_crypt": ("test_gpu_crypt", "test_adx_crypt_matches_oracle", (7, 100, 9)),
        "hca_crypt": ("test_gpu_crypt", "test_hca_crypt_matches_oracle", (88888888,)),
        "adx_find_key": ("test_gpu_crypt", "test_adx_find_key", ()),
        "adx_guess_keys": ("test_gpu_crypt", "test_adx_guess_keys_matches_oracle_and_finds_the_key", ()),
        "hca_find_key": ("test_gpu_crypt", "test_hca_find_key_matches_oracle", ()),
        "hca_stream": ("test_gpu_hca", "test_streaming_encoder_object_matches_the_batch_encoder_and_the_reference_call_pattern",
                       (2, "High", 20000, (3000, 18000))),
        "dsptool": ("test_gpu_gcadpcm", "test_dsptool_compatible_exports", ()),
    }


HOST_CHECK_NAMES = [
    "dsp_file", "dsp_looping_file", "dsp_round_trip", "adx_file", "adx_round_trip", "adx_encrypted_files", "hca_file",
    "hca_round_trip", "hca_encrypted_files", "brstm_gc", "bcstm_gc", "bfstm_gc", "brstm_pcm16", "bcstm_pcm8", "bfstm_pcm8", "hps",
    "hps_unaligned_loop", "idsp", "genh", "wave16", "wave16_file", "wave8_file", "nwwav_bank", "nwwav_bank_rows",
    "nwwav_prefetch_bank", "gc_build_channels_loops", "gc_build_channels_shift", "gc_coefs", "gc_encode_with_coefs", "gc_ragged_with_coefs", "adx_crypt",
    "hca_crypt", "adx_find_key", "adx_guess_keys", "hca_find_key", "hca_stream", "dsptool"]

# the host-pointer functions of the headers that HOST_CHECKS drive (test (c) holds the GPU run to it)
HOST_COVERED = {
    "vga_dsp_write", "vga_dsp_read", "vga_adx_write", "vga_adx_read", "vga_hca_write", "vga_hca_read",
    "vga_nwstm_write", "vga_nwstm_read", "vga_nwstm_pcm_write", "vga_nwstm_pcm_read", "vga_hps_write", "vga_hps_read",
    "vga_idsp_write", "vga_idsp_read", "vga_genh_read", "vga_wave_write_pcm16", "vga_wave_read_pcm16", "vga_wave_write_pcm8",
    "vga_wave_read_pcm8", "vga_nwwav_bank_create", "vga_nwwav_bank_read_device", "vga_gcadpcm_build_channels_batch",
    "vga_gcadpcm_calculate_coefficients_batch", "vga_gcadpcm_encode_with_coefs_batch", "vga_gcadpcm_encode_with_coefs_batch_v",
    "vga_gcadpcm_ragged_create",
    "vga_adx_crypt", "vga_hca_crypt", "vga_adx_guess_keys", "vga_hca_find_key", "vga_hca_stream_create", "vga_hca_stream_encode",
    "encode", "decode", "correlateCoefs", "encodeFrame",
}


def _hp():
    import test_gpu_host_paths as hp
    return hp


@pytest.mark.gpu
@pytest.mark.parametrize("byte", POISON_BYTES)
@pytest.mark.parametrize("shape", ["direct", "staged"])
@pytest.mark.parametrize("name", list(BATCH_CASES))
def test_batch_entry_point_on_poisoned_memory(name, shape, byte):
    hp = _hp()
    c = hp.case(name)
    with poisoned(byte), hp.hooks(**hp.SHAPES[shape]):
        c.run((shape, hex(byte)))
    RAN.add(name)


def test_batch_cases_are_those_of_the_host_path_table():
    assert set(BATCH_CASES) == set(_hp().CASES)
    assert list(_host_checks()) == HOST_CHECK_NAMES


@pytest.mark.gpu
@pytest.mark.parametrize("byte", POISON_BYTES)
@pytest.mark.parametrize("name", HOST_CHECK_NAMES)
def test_host_pointer_call_on_poisoned_memory(name, byte):
    import importlib
    module, function, args = _host_checks()[name]
    check = getattr(importlib.import_module(module), function)
    with poisoned(byte):
        check(*args)
    RAN.add(name)


# ---------------------------------------------------------------- b. device entry points: poisoned scratch, junk padding
# Rows whose header text REQUIRES a region of an input to hold defined values get zeros there instead of junk:
# entry point -> the header line that says so.  (NULL history pointers mean zero history by the header -- "or NULL for 0",
# include/vgaudio_hip.h -- and name no memory; the 8 bytes of slack behind the frames of vga_hca_decode_device only have to
# exist: "with >= 8 bytes of slack after frame_count*frame_size", include/vgaudio_hip.h.  Both run with junk.)
DEFINED_PADDING = {}


def _device_rows():
    import test_gpu_pcm_device_streams as pds
    rows = {name: (lambda k, shared, make=make: make(k, shared)) for name, make in ds.ROWS.items()}
    rows.update({name + "[seams]": (lambda k, shared, make=make: make(k, shared)) for name, make in ds.SEAM_ROWS.items()})
    rows.update({name: (lambda k, shared, make=make: make(k)) for name, make in pds.ROWS.items()})
    return rows


DEVICE_ROW_NAMES = sorted(ds.ROWS) + [n + "[seams]" for n in sorted(ds.SEAM_ROWS)] + [
    "vga_nwstm_pcm_read_device", "vga_nwstm_pcm_write_device", "vga_pcm8_decode_device", "vga_pcm8_encode_device",
    "vga_wave_deinterleave_pcm8_device", "vga_wave_write_pcm8_device"]


def test_device_rows_are_those_of_the_two_stream_tables():
    assert sorted(_device_rows()) == sorted(DEVICE_ROW_NAMES)
    assert set(DEFINED_PADDING) <= set(DEVICE_ROW_NAMES)


@pytest.mark.gpu
@pytest.mark.parametrize("byte", POISON_BYTES)
@pytest.mark.parametrize("name", DEVICE_ROW_NAMES)
def test_device_entry_point_with_poisoned_scratch_and_junk_padding(name, byte):
    import torch
    make = _device_rows()[name]
    shared = {}
    S = torch.cuda.Stream()
    ds._hooks(name.endswith("[seams]"))
    try:
        with poisoned(byte):
            with ds.pad_fill(0 if name in DEFINED_PADDING else ds.JUNK):
                case = make(0, shared)                      # (a ragged handle is created here: its tables are poisoned first)
            with torch.cuda.stream(S):
                case.poison()
                case.load()                                 # the real rows, with the junk behind them
            rc = case.call(S.cuda_stream)
            S.synchronize()
        ds._ok(rc)
        case.check()
        assert case.inputs_unchanged(), f"{name}: the call changed an input byte (padding included)"
    finally:
        ds._hooks(False)
        torch.cuda.synchronize()
        if "ragged" in shared:
            shared["ragged"].close()
    RAN.add(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ds.ROWS) + [n + "[seams]" for n in sorted(ds.SEAM_ROWS)])
def test_busy_stream_test_in_poison_mode(name, delay):  # noqa: F811
    """test_gpu_device_streams.test_device_entry_point_on_a_busy_stream as it is, with every allocation poisoned: the
    stream-ordered fill must not make an entry point wait for the caller's stream"""
    with poisoned(0xA5):
        ds.test_device_entry_point_on_a_busy_stream(name, delay)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ds.CONCURRENT)
def test_two_calls_in_flight_in_poison_mode(name, delay):  # noqa: F811
    with poisoned(0xA5):
        ds.test_two_calls_in_flight(name, delay)


@pytest.mark.gpu
@pytest.mark.parametrize("name", DEVICE_ROW_NAMES[-6:])
def test_pcm_busy_stream_test_in_poison_mode(name, delay):  # noqa: F811
    import test_gpu_pcm_device_streams as pds
    with poisoned(0xA5):
        pds.test_pcm_device_entry_point_on_a_busy_stream(name, delay)


# ---------------------------------------------------------------- c. completeness
# Functions that allocate no device or page-locked memory and launch nothing: host arithmetic, parsers of host bytes,
# accessors of host-side handles, process settings, test hooks.
_ARITHMETIC = "host arithmetic on its arguments"
_PARSER = "parses or lays out host bytes; no device memory"
_ACCESSOR = "reads or frees a host-side handle; allocates and launches nothing"
_SETTING = "process or thread setting; host state"
_HOOK = "test hook; host state or host arithmetic"
EXEMPT = {
    **{n: _ARITHMETIC for n in (
        "vga_gcadpcm_nibble_count_to_sample_count", "vga_gcadpcm_sample_count_to_nibble_count", "vga_gcadpcm_nibble_to_sample",
        "vga_gcadpcm_sample_to_nibble", "vga_gcadpcm_sample_count_to_byte_count", "vga_gcadpcm_byte_count_to_sample_count",
        "vga_gcadpcm_coefs_workspace_bytes", "vga_gcadpcm_build_channels_workspace_bytes", "vga_gcadpcm_channel_layout_for",
        "vga_adx_default_params", "vga_adx_calculate_coefficients", "vga_adx_nibble_count_to_sample_count",
        "vga_adx_sample_count_to_nibble_count", "vga_adx_sample_count_to_byte_count", "vga_adx_encoded_byte_count",
        "vga_adx_key_from_code", "vga_adx_key_from_string", "vga_adx_key_code", "vga_adx_guess_default_candidates",
        "vga_hca_encoder_initialize", "vga_hca_decode_workspace_bytes", "vga_hca_file_size", "vga_hca_key_tables",
        "vga_wave_file_size", "vga_wave_pcm8_file_size")},
    **{n: _PARSER for n in (
        "vga_dsp_layout_for", "vga_dsp_parse", "vga_nwstm_layout_for", "vga_nwstm_parse", "vga_nwstm_pcm_layout_for",
        "vga_nwstm_pcm_parse", "vga_hps_layout_for", "vga_hps_block_map", "vga_hps_parse", "vga_idsp_layout_for", "vga_idsp_parse",
        "vga_genh_parse", "vga_adx_file_layout_for", "vga_adx_parse", "vga_hca_file_header", "vga_hca_parse", "vga_wave_parse",
        "vga_nwwav_parse", "vga_nwwav_read")},
    **{n: _ACCESSOR for n in (
        "vga_gcadpcm_ragged_destroy", "vga_gcadpcm_ragged_channels", "vga_gcadpcm_ragged_pcm_samples",
        "vga_gcadpcm_ragged_adpcm_bytes", "vga_gcadpcm_ragged_coefs_workspace_bytes", "vga_gcadpcm_ragged_offsets",
        "vga_hca_stream_pending_frame_count", "vga_hca_stream_get_pending_frame", "vga_hca_stream_frames_processed",
        "vga_hca_stream_frame_size", "vga_hca_stream_destroy", "vga_nwwav_bank_destroy", "vga_nwwav_bank_channels",
        "vga_nwwav_bank_codec_channels", "vga_nwwav_bank_rows", "vga_nwwav_bank_gc_sample_counts", "vga_nwwav_bank_gc_tables",
        "vga_nwwav_bank_adpcm_bytes", "vga_nwwav_bank_pcm16_samples", "vga_nwwav_bank_pcm8_bytes",
        "vga_nwwav_bank_source_bytes")},
    **{n: _SETTING for n in (
        "vga_last_error", "vga_version", "vga_device_count", "vga_set_device", "vga_set_devices", "vga_get_devices",
        "vga_set_progress_callback", "vga_release_cached_memory")},
}


def _header_functions():
    return set(_declared_symbols())


def _device_covered():
    return {n for n in DEVICE_ROW_NAMES if not n.endswith("[seams]")}


def test_every_header_function_is_covered_or_exempt():
    declared = _header_functions()
    assert len(declared) >= 170
    hooks = {n for n in declared if n.startswith("vga_testing_")}
    covered = set(BATCH_CASES.values()) | HOST_COVERED | _device_covered()
    assert not covered & set(EXEMPT), sorted(covered & set(EXEMPT))
    assert not hooks & (covered | set(EXEMPT)), "test hooks are exempt as a class"
    missing = declared - covered - set(EXEMPT) - hooks
    stale = (covered | set(EXEMPT)) - declared
    assert not missing, f"neither exercised on dirty memory nor exempt: {sorted(missing)}"
    assert not stale, f"not in the headers: {sorted(stale)}"
    assert all(isinstance(r, str) and r for r in EXEMPT.values())


def test_no_exempt_function_allocates():
    """EXEMPT may hold only functions that allocate and launch nothing: none of their definitions (up to the closing brace in
    column 0) names an allocator, a launch, a pipeline or a device entry point"""
    import re
    csrc = os.path.join(ROOT, "vgaudio_amd", "csrc")
    text = "\n".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(".hip"))
    busy = re.compile(r"DevBuf|AsyncBuf|PinnedBlock|device_malloc|hipMalloc|hipHostMalloc|hipLaunchKernelGGL|<<<|launch_\w+\(|pipe::run|"
                      r"vga_\w+_device(?:_v)?\(|vga_\w+_batch(?:_v)?\(")
    bad, found = [], 0
    for name in EXEMPT:
        m = re.search(r"^[A-Za-z_][\w \*]*\b" + name + r"\s*\([^;{]*\)\s*\{", text, flags=re.M)
        if not m:
            continue
        found += 1
        line = text[m.end():text.find("\n", m.end())]
        body = line if line.rstrip().endswith("}") else text[m.end():text.find("\n}", m.end())]
        if busy.search(body):
            bad.append(name)
    assert found >= len(EXEMPT) * 3 // 4, (found, len(EXEMPT))
    assert not bad, f"EXEMPT functions whose definitions allocate or launch: {bad}"


@pytest.mark.gpu
def test_the_gpu_run_called_every_covered_function_in_poison_mode():
    """runs last: what (a) and (b) claim to cover was really fetched from the library while the mode was on (only when every
    driver ran in this process: a run of selected tests proves nothing here)"""
    everything = set(BATCH_CASES) | set(HOST_CHECK_NAMES) | set(DEVICE_ROW_NAMES)
    if RAN != everything:
        assert RAN < everything
        print(f"\n[dirty memory] {len(RAN)} of {len(everything)} drivers ran in this process: coverage not judged")
        return
    covered = set(BATCH_CASES.values()) | HOST_COVERED | _device_covered()
    print("\n[dirty memory] called in poison mode:", " ".join(sorted(CALLED)))
    assert not covered - CALLED, f"claimed but never called in poison mode: {sorted(covered - CALLED)}"
    uncounted = (CALLED & _header_functions()) - covered - set(EXEMPT)
    assert all(n.startswith("vga_testing_") for n in uncounted), sorted(uncounted)


# ---------------------------------------------------------------- d. the product path: the hook off, blocks handed between codecs
def _noise(nch, n, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, (nch, n)).astype(np.int16)


def _signal(call, nch, n, seed):
    """call 0: full-scale white noise; later calls: the synthetic channels"""
    from oracle import pyoracle as po
    return _noise(nch, n, seed) if call == 0 else po.synth_generate(nch, n, first_channel=seed)


SCALE = [1.0, 0.75, 0.62]       # a later request of 0.6 .. 0.9 of the first gets the first call's block (the pool's half-size rule)
MIB = 1 << 20


def _gc_call(call):
    from oracle import pyoracle as po
    hp = _hp()
    nch, n = 16, 14 * int(15000 * SCALE[call]) + 5            # = 5 (mod 14): a last frame of 5 samples
    pcm = _signal(call, nch, n, 3000 + call)
    wc, wa = po.gc_encode_batch(pcm, threads=8)
    assert nch * wa.shape[1] >= MIB and pcm.nbytes >= MIB
    c = hp.Case()
    c.units = nch
    c.setup(hp.in_rows(list(pcm), hp.EVEN), [wa.shape[1]] * nch, hp.ALL, list(wa), np.uint8)
    coefs = c.host(nch * 16, np.int16, 0x5A5A, wc.reshape(-1))
    c.call = lambda: hp.L().vga_gcadpcm_encode_batch(c.ins.ptrs(hp.i16p), nch, n, 0, 0, coefs.ctypes.data_as(hp.i16p), c.outs.ptrs(hp.u8p))
    c.run(("gc", call))


def _adx_call(call):
    from oracle import pyoracle as po
    hp = _hp()
    nch, n = 16, 32 * int(6600 * SCALE[call]) + 5             # = 5 (mod 32)
    pcm = _signal(call, nch, n, 4000 + call)
    want, hist = po.adx_encode_batch(pcm, po.adx_params(), threads=8)
    assert nch * want.shape[1] >= MIB and pcm.nbytes >= MIB
    p = hp.adx_params()
    c = hp.Case()
    c.units = nch
    c.setup(hp.in_rows(list(pcm), hp.EVEN), [want.shape[1]] * nch, hp.ALL, list(want), np.uint8)
    h = c.host(nch, np.int16, 0x3C3C, hist)
    c.call = lambda: hp.L().vga_adx_encode_batch(c.ins.ptrs(hp.i16p), nch, n, C.byref(p), c.outs.ptrs(hp.u8p), h.ctypes.data_as(hp.i16p))
    c.run(("adx", call))


def _hca_call(call):
    from oracle import pyoracle as po
    hp = _hp()
    nch, n = 2, int(120000 * SCALE[call]) + 77
    cp, info = hp.hca_info(nch, n)
    ns = -(-int(1.05 * MIB) // (info.frame_count * info.frame_size))
    pcm = _signal(call, ns * nch, n, 5000 + call).reshape(ns, nch, n)
    rc, _, want = po.hca_encode_batch(pcm, po.hca_params(nch, n), threads=8)
    assert rc == 0 and want.size >= MIB
    c = hp.Case()
    c.units = ns
    c.setup(hp.in_rows([pcm[s, ch] for s in range(ns) for ch in range(nch)], hp.EVEN), [want.shape[1]] * ns, hp.ALL, list(want), np.uint8)
    out_info = _lib().HcaInfoC()
    c.call = lambda: hp.L().vga_hca_encode_batch(c.ins.ptrs(hp.i16p), ns, C.byref(cp), C.byref(out_info), c.outs.ptrs(hp.u8p))
    c.run(("hca", call))


def _reader_call(call):
    """the DSP file reader (vga_dsp_read), images of 2 MiB and more"""
    import test_gpu_container_readers as readers
    readers.test_dsp_round_trip(2, 14 * int(140000 * SCALE[call]) + 5, call == 1)


def _bank_call(call):
    import test_gpu_nwwav as nw
    nw.check_bank(nw.make_bank(600 + call, int(40 * SCALE[call]), [int(300000 * SCALE[call]), 16385, None, int(250001 * SCALE[call])]))


FAMILIES = {"gc": _gc_call, "adx": _adx_call, "hca": _hca_call, "reader": _reader_call, "bank": _bank_call}


@pytest.mark.gpu
def test_pool_blocks_handed_between_codecs_with_the_hook_off():
    import torch
    import test_gpu_hca as th
    import test_gpu_nwwav as nw
    from oracle import pyoracle as po
    from vgaudio_amd.crihca import CriHcaEncoder, CriHcaParameters
    from vgaudio_amd.nwwav import NwWaveBank
    assert _setting() == -1
    _lib().lib().vga_release_cached_memory()                 # the sequence starts from an empty pool: its own blocks travel
    # persistent handles, opened before the sequence and used again after it
    shared = {}
    first = ds.row_gc_encode_v(0, shared)                    # the ragged batch (shared["ragged"])
    ds._ok(first.call(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    first.check()
    files = nw.make_bank(77, 30, [20000, None, 16385])
    bank = NwWaveBank([img for img, _ in files])
    nch, n = 2, 20000
    stream = th._streams(1, nch, n, "synth")[0]
    rc, _, want = po.hca_encode(stream, po.hca_params(nch, n, quality="High"))
    assert rc == 0
    enc = CriHcaEncoder.InitializeNew(CriHcaParameters(Quality=th.Q["High"], ChannelCount=nch, SampleRate=48000, SampleCount=n))
    blocks = -(-n // 1024)
    frames, out = [], np.zeros(enc.FrameSize, np.uint8)

    def feed(lo, hi):
        """blocks lo..hi-1 of 1024 samples, as test_gpu_hca._feed hands them over"""
        for b in range(lo, hi):
            buf = np.zeros((nch, 1024), dtype=np.int16)
            piece = stream[:, b * 1024:(b + 1) * 1024]
            buf[:, :piece.shape[1]] = piece
            got = enc.Encode(list(buf), out)
            if got:
                frames.append(out.copy())
                while enc.PendingFrameCount:
                    frames.append(enc.GetPendingFrame())
    try:
        feed(0, blocks // 2)
        order = [(f, k) for k in range(3) for f in np.random.default_rng(1234 + k).permutation(sorted(FAMILIES))]
        for family, k in order:
            FAMILIES[family](k)
        # the handles again
        feed(blocks // 2, blocks)
        tail = blocks
        while enc.FramesProcessed < enc.Hca.FrameCount:      # (the frames behind the last block of PCM)
            feed(tail, tail + 1)
            tail += 1
        got = np.stack(frames)
        assert got.shape == want.shape and np.array_equal(got, want), "HCA stream object"
        again = ds.row_gc_encode_v(1, shared)
        ds._ok(again.call(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        again.check()
        pcm = bank.decode_to_pcm16()
        import nwwav_ref as ref
        for f, (img, given) in enumerate(files):
            s = ref.read_image(img)
            for c in range(s["nch"]):
                if s["codec"] == ref.GCADPCM:
                    ch = s["channels"][c]
                    w = po.gc_decode(np.frombuffer(s["audio"][c], dtype=np.uint8), np.array(ch["coefs"], dtype=np.int16),
                                     s["sample_count"], ch["start"][1], ch["start"][2])
                elif s["codec"] == ref.PCM16:
                    w = np.frombuffer(given["audio"][c], dtype=">i2" if s["big"] else "<i2").astype(np.int16)
                else:
                    w = np.frombuffer(given["audio"][c], dtype=np.int8).astype(np.int16) << 8
                assert np.array_equal(pcm[f][c], w), ("bank", f, c)
    finally:
        enc.close()
        bank.close()
        shared["ragged"].close()
        torch.cuda.synchronize()

"""ctypes binding of libvgaudio_hip.so (the C ABI in include/vgaudio_hip.h).

There is no CPU fallback: if the shared library is missing or no HIP device is
visible, calls fail loudly (VgaError / OSError).
"""
import ctypes as C
import importlib.util
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# VGAUDIO_HIP_LIBRARY: load a different build of the same ABI (kernel experiments, tools/variants/)
SO_PATH = os.environ.get("VGAUDIO_HIP_LIBRARY") or os.path.join(_HERE, "libvgaudio_hip.so")

VGA_OK = 0
VGA_ERR_ARGUMENT = -1
VGA_ERR_OUT_OF_RANGE = -2
VGA_ERR_INVALID_DATA = -3
VGA_ERR_INVALID_OP = -4
VGA_ERR_DEVICE = -5

# step kinds of vga_testing_fail_step_this_thread (include/vgaudio_hip_testing.h)
VGA_TESTING_STEP_CHUNK_COMPUTE = 1
VGA_TESTING_STEP_TRANSFER = 2
VGA_TESTING_STEP_HCA_STREAM_FRAMES = 3


class VgaError(RuntimeError):
    """Base class; subclasses mirror the .NET exception the reference throws."""
    code = None


class ArgumentError(VgaError, ValueError):           # ArgumentException
    code = VGA_ERR_ARGUMENT


class ArgumentOutOfRangeError(ArgumentError):        # ArgumentOutOfRangeException
    code = VGA_ERR_OUT_OF_RANGE


class InvalidDataError(VgaError):                    # InvalidDataException
    code = VGA_ERR_INVALID_DATA


class InvalidOperationError(VgaError):               # InvalidOperationException
    code = VGA_ERR_INVALID_OP


class DeviceError(VgaError):                         # HIP failure / no device
    code = VGA_ERR_DEVICE


PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_int64)     # vga_progress_fn


class reporting:
    """`with reporting(progress, frames_per_unit):` around a *_batch call: IProgressReport.ReportAdd once per chunk of
    channels / streams the call finishes (vga_set_progress_callback), where the reference reports once per frame
    (GcAdpcmEncoder.cs:42, CriAdxCodec.cs:101, CriHcaFormat.cs:71,79).  progress None: nothing is installed."""

    def __init__(self, progress, per_unit):
        self.progress, self.per_unit, self.last, self.fn = progress, per_unit, 0, None

    def _report(self, _user, done, _total):
        self.progress.ReportAdd((done - self.last) * self.per_unit)
        self.last = done

    def __enter__(self):
        if self.progress is not None:
            self.fn = PROGRESS_FN(self._report)
            lib().vga_set_progress_callback(C.cast(self.fn, C.c_void_p), None)
        return self

    def __exit__(self, *exc):
        if self.fn is not None:
            lib().vga_set_progress_callback(None, None)
        return False


_EXC = {e.code: e for e in (ArgumentError, ArgumentOutOfRangeError, InvalidDataError, InvalidOperationError,
                            DeviceError)}

_lib = None

i16p = C.POINTER(C.c_int16)
u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
i16pp = C.POINTER(i16p)
u8pp = C.POINTER(u8p)
vp = C.c_void_p
i64 = C.c_int64
ci = C.c_int


class ADPCMINFO(C.Structure):
    _pack_ = 1
    _fields_ = [("coef", C.c_int16 * 16), ("gain", C.c_uint16), ("pred_scale", C.c_uint16), ("yn1", C.c_int16),
                ("yn2", C.c_int16), ("loop_pred_scale", C.c_uint16), ("loop_yn1", C.c_int16), ("loop_yn2", C.c_int16)]


# name -> (restype, argtypes); every symbol include/vgaudio_hip.h declares
SIGNATURES = {
    "vga_last_error": (C.c_char_p, []),
    "vga_device_count": (ci, []),
    "vga_set_device": (ci, [ci]),
    "vga_version": (C.c_char_p, []),
    "vga_gcadpcm_nibble_count_to_sample_count": (ci, [ci]),
    "vga_gcadpcm_sample_count_to_nibble_count": (ci, [ci]),
    "vga_gcadpcm_nibble_to_sample": (ci, [ci]),
    "vga_gcadpcm_sample_to_nibble": (ci, [ci]),
    "vga_gcadpcm_sample_count_to_byte_count": (ci, [ci]),
    "vga_gcadpcm_byte_count_to_sample_count": (ci, [ci]),
    "vga_gcadpcm_encode_batch": (ci, [i16pp, ci, ci, C.c_int16, C.c_int16, i16p, u8pp]),
    "vga_gcadpcm_calculate_coefficients_batch": (ci, [i16pp, ci, ci, i16p]),
    "vga_gcadpcm_encode_with_coefs_batch": (ci, [i16pp, ci, ci, ci, i16p, i16p, i16p, u8pp]),
    "vga_gcadpcm_decode_batch": (ci, [u8pp, i16p, ci, ci, i16p, i16p, i16pp]),
    "vga_gcadpcm_encode_batch_v": (ci, [i16pp, C.POINTER(ci), ci, i16p, i16p, i16p, u8pp]),
    "vga_gcadpcm_calculate_coefficients_batch_v": (ci, [i16pp, C.POINTER(ci), ci, i16p]),
    "vga_gcadpcm_encode_with_coefs_batch_v": (ci, [i16pp, C.POINTER(ci), ci, i16p, i16p, i16p, u8pp]),
    "vga_gcadpcm_decode_batch_v": (ci, [u8pp, i16p, C.POINTER(ci), ci, i16p, i16p, i16pp]),
    "vga_gcadpcm_ragged_create": (ci, [C.POINTER(ci), ci, C.POINTER(vp)]),
    "vga_gcadpcm_ragged_destroy": (None, [vp]),
    "vga_gcadpcm_ragged_channels": (ci, [vp]),
    "vga_gcadpcm_ragged_pcm_samples": (i64, [vp]),
    "vga_gcadpcm_ragged_adpcm_bytes": (i64, [vp]),
    "vga_gcadpcm_ragged_coefs_workspace_bytes": (C.c_size_t, [vp]),
    "vga_gcadpcm_ragged_offsets": (ci, [vp, C.POINTER(i64), C.POINTER(i64)]),
    "vga_gcadpcm_coefs_device_v": (ci, [vp, vp, vp, vp, C.c_size_t, vp]),
    "vga_gcadpcm_encode_device_v": (ci, [vp, vp, vp, vp, vp, vp, vp]),
    "vga_gcadpcm_decode_device_v": (ci, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "encode": (None, [i16p, u8p, C.POINTER(ADPCMINFO), C.c_uint32]),
    "decode": (None, [u8p, i16p, C.POINTER(ADPCMINFO), C.c_uint32]),
    "correlateCoefs": (None, [i16p, C.c_uint32, i16p]),
    "encodeFrame": (None, [i16p, u8p, i16p, C.c_uint8]),
    "vga_gcadpcm_coefs_workspace_bytes": (C.c_size_t, [ci, ci]),
    "vga_gcadpcm_coefs_device": (ci, [vp, i64, ci, ci, vp, vp, C.c_size_t, vp]),
    "vga_gcadpcm_encode_device": (ci, [vp, i64, ci, ci, vp, vp, vp, vp, i64, vp]),
    "vga_gcadpcm_decode_device": (ci, [vp, i64, vp, ci, ci, vp, vp, vp, i64, vp, vp]),
    "vga_synth_pcm16_device": (ci, [vp, i64, ci, ci, ci, vp, vp]),
    "vga_adx_file_layout_for": (ci, [vp, ci, vp]),
    "vga_adx_write": (ci, [u8pp, ci, i16p, ci, vp, u8p]),
    "vga_adx_write_device": (ci, [vp, i64, ci, vp, ci, vp, vp, vp]),
    "vga_hca_file_size": (ci, [vp]),
    "vga_hca_file_header": (ci, [vp, C.c_char_p, C.c_float, ci, ci, u8p]),
    "vga_hca_write": (ci, [vp, u8p, C.c_char_p, C.c_float, ci, ci, u8p]),
    "vga_hca_write_device": (ci, [vp, vp, i64, ci, C.c_char_p, C.c_float, ci, ci, vp, i64, vp]),
    "vga_wave_parse": (ci, [u8p, i64, vp]),
    "vga_wave_read_pcm16": (ci, [u8p, i64, vp, i16pp]),
    "vga_wave_deinterleave_pcm16_device": (ci, [vp, ci, ci, vp, i64, vp]),
    "vga_wave_file_size": (i64, [vp, ci]),
    "vga_wave_write_pcm16": (ci, [i16pp, ci, vp, u8p]),
    "vga_wave_write_pcm16_device": (ci, [vp, i64, ci, vp, vp, vp]),
    "vga_adx_key_from_code": (ci, [C.c_uint64, vp]),
    "vga_adx_key_from_string": (ci, [C.c_char_p, vp]),
    "vga_adx_key_code": (C.c_uint64, [vp]),
    "vga_adx_crypt": (ci, [u8pp, ci, ci, vp, ci, ci]),
    "vga_adx_crypt_device": (ci, [vp, i64, ci, ci, vp, ci, ci, vp]),
    "vga_adx_find_key_device": (ci, [vp, i64, ci, ci, ci, ci, vp, ci, C.POINTER(ci), vp]),
    "vga_hca_key_tables": (ci, [ci, C.c_uint64, u8p, u8p]),
    "vga_hca_crypt": (ci, [u8p, ci, ci, u8p]),
    "vga_hca_find_key": (ci, [vp, u8p, ci, u8p, ci, vp]),
    "vga_hca_find_key_device": (ci, [vp, vp, ci, u8p, ci, vp, vp]),
    "vga_hca_byte_position_counts_device": (ci, [vp, i64, ci, ci, ci, ci, vp, vp]),
    "vga_adx_guess_default_candidates": (ci, [ci, vp, vp, vp, vp]),
    "vga_adx_guess_keys": (ci, [vp, ci, ci, ci, vp, ci, vp, ci, vp, ci, vp]),
    "vga_hca_crypt_device": (ci, [vp, i64, ci, ci, ci, u8p, vp]),
    "vga_release_cached_memory": (None, []),
    "vga_testing_force_open_seams_this_thread": (ci, [ci]),
    "vga_testing_host_pipeline_this_thread": (None, [ci, ci, ci, ci]),
    "vga_testing_gc_encoder_layout_this_thread": (ci, [ci]),
    "vga_testing_gc_coefs_variant_this_thread": (ci, [ci]),
    "vga_testing_gc_encoder_segments_this_thread": (ci, [ci]),
    "vga_testing_gc_encoder_persistent_this_thread": (ci, [ci]),
    "vga_testing_gc_seam_handover_this_thread": (ci, [ci]),
    "vga_testing_gc_schedule_this_thread": (ci, [ci, C.POINTER(ci), C.POINTER(ci), ci]),
    "vga_testing_gc_slow_order_host": (ci, [vp, ci, vp]),
    "vga_testing_gc_slow_order_device": (ci, [vp, ci, vp]),
    "vga_testing_gc_prologue_device": (ci, [vp, ci, ci, vp, vp]),
    "vga_testing_gc_encode_stats_n": (ci, [C.POINTER(C.c_ulonglong), ci, ci]),
    "vga_testing_last_pipeline_stats": (ci, [vp, ci]),
    "vga_testing_host_pipeline_tail_this_thread": (None, [ci]),
    "vga_testing_buckets_order_this_thread": (None, [ci]),
    "vga_testing_host_transfer_this_thread": (None, [ci]),
    "vga_testing_host_transfer_piece_bytes_this_thread": (None, [ci]),
    "vga_testing_host_compute_lanes_this_thread": (None, [ci]),
    "vga_testing_fail_step_this_thread": (None, [ci, ci]),
    "vga_testing_poison_allocations": (ci, [ci]),
    "vga_testing_plan_buckets": (ci, [C.POINTER(ci), C.POINTER(ci), ci, ci, C.c_longlong, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci),
                                 C.POINTER(ci), ci]),
    "vga_testing_hca_device_info": (ci, [vp, vp, ci]),
    "vga_testing_hca_decode_classes": (ci, [vp, ci, C.POINTER(ci)]),
    "vga_testing_hca_decode_v_stats": (ci, [C.POINTER(C.c_longlong), ci]),
    "vga_testing_hca_ragged_stats": (ci, [vp, C.POINTER(C.c_longlong), ci]),
    "vga_hca_ragged_layout_for": (ci, [vp, ci, C.POINTER(i64), C.POINTER(i64), vp]),
    "vga_hca_ragged_create": (ci, [vp, ci, C.POINTER(vp)]),
    "vga_hca_ragged_destroy": (None, [vp]),
    "vga_hca_ragged_streams": (ci, [vp]),
    "vga_hca_ragged_totals_of": (ci, [vp, vp]),
    "vga_hca_ragged_offsets": (ci, [vp, C.POINTER(i64), C.POINTER(i64)]),
    "vga_testing_adx_ragged_stats": (ci, [vp, C.POINTER(C.c_longlong), ci]),
    "vga_adx_ragged_layout_for": (ci, [vp, C.POINTER(ci), ci, C.POINTER(i64), C.POINTER(i64), vp]),
    "vga_adx_ragged_create": (ci, [vp, C.POINTER(ci), ci, C.POINTER(vp)]),
    "vga_adx_ragged_destroy": (None, [vp]),
    "vga_adx_ragged_channels": (ci, [vp]),
    "vga_adx_ragged_totals_of": (ci, [vp, vp]),
    "vga_adx_ragged_offsets": (ci, [vp, C.POINTER(i64), C.POINTER(i64)]),
    "vga_adx_encode_device_v": (ci, [vp, vp, vp, vp, vp, C.c_size_t, vp]),
    "vga_adx_decode_device_v": (ci, [vp, vp, vp, vp, C.c_size_t, vp, vp]),
    # include/vgaudio_hip/gc_files.h
    "vga_gc_files_layout_for": (ci, [vp, ci, vp, C.POINTER(ci), C.POINTER(i64), C.POINTER(i64), vp]),
    "vga_gc_files_create": (ci, [vp, ci, vp, C.POINTER(vp)]),
    "vga_gc_files_create_from_dsp": (ci, [C.POINTER(vp), ci, C.POINTER(i64), C.POINTER(vp)]),
    "vga_gc_files_destroy": (None, [vp]),
    "vga_gc_files_totals_of": (ci, [vp, vp]),
    "vga_gc_files_offsets": (ci, [vp, C.POINTER(ci), C.POINTER(i64), C.POINTER(i64)]),
    "vga_gc_files_ragged": (vp, [vp]),
    "vga_gcadpcm_build_channels_device_v": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]),
    "vga_dsp_write_device_v": (ci, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "vga_dsp_read_device_v": (ci, [vp, vp, vp, vp, vp, vp, vp, vp]),
    # include/vgaudio_hip/gc_files_aligned.h
    "vga_gc_aligned_layout_for": (ci, [vp, ci, C.POINTER(ci), C.POINTER(i64), vp]),
    "vga_gc_aligned_create": (ci, [vp, ci, C.POINTER(vp)]),
    "vga_gc_aligned_destroy": (None, [vp]),
    "vga_gc_aligned_totals_of": (ci, [vp, vp]),
    "vga_gc_aligned_offsets": (ci, [vp, C.POINTER(ci), C.POINTER(i64)]),
    "vga_gc_aligned_ragged_in": (vp, [vp]),
    "vga_gc_aligned_ragged_out": (vp, [vp]),
    "vga_gcadpcm_align_channels_device_v": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]),
    # include/vgaudio_hip/nw_files.h
    "vga_nw_files_layout_for": (ci, [vp, ci, vp, C.POINTER(ci), C.POINTER(i64), C.POINTER(i64), vp]),
    "vga_nw_files_create": (ci, [vp, ci, vp, C.POINTER(vp)]),
    "vga_nw_files_create_from_infos": (ci, [C.POINTER(vp), ci, C.POINTER(i64), C.POINTER(vp)]),
    "vga_nw_files_destroy": (None, [vp]),
    "vga_nw_files_totals_of": (ci, [vp, vp]),
    "vga_nw_files_offsets": (ci, [vp, C.POINTER(ci), C.POINTER(i64), C.POINTER(i64)]),
    "vga_nw_files_gc_files": (ci, [vp, vp]),
    "vga_nw_files_ragged": (vp, [vp]),
    "vga_nwstm_write_device_v": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "vga_nwstm_read_device_v": (ci, [vp, vp, vp, vp, vp, vp, vp, vp]),
    # include/vgaudio_hip_files/idsp_files.h
    "vga_idsp_files_layout_for": (ci, [vp, ci, vp, C.POINTER(ci), C.POINTER(i64), vp]),
    "vga_idsp_files_create": (ci, [vp, ci, vp, C.POINTER(vp)]),
    "vga_idsp_files_create_from_infos": (ci, [C.POINTER(vp), ci, C.POINTER(i64), C.POINTER(vp)]),
    "vga_idsp_files_destroy": (None, [vp]),
    "vga_idsp_files_totals_of": (ci, [vp, vp]),
    "vga_idsp_files_offsets": (ci, [vp, C.POINTER(ci), C.POINTER(i64)]),
    "vga_idsp_files_gc_files": (ci, [vp, vp]),
    "vga_idsp_files_ragged": (vp, [vp]),
    "vga_idsp_write_device_v": (ci, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "vga_idsp_read_device_v": (ci, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "vga_idsp_files_write_regions_for": (ci, [vp, ci, vp, vp, i64, C.POINTER(i64)]),
    "vga_idsp_files_read_regions_for": (ci, [C.POINTER(vp), ci, C.POINTER(i64), vp, i64, C.POINTER(i64)]),
    "vga_idsp_files_stats": (ci, [vp, C.POINTER(i64)]),
    # include/vgaudio_hip_files/hps_files.h
    "vga_hps_files_layout_for": (ci, [vp, ci, C.POINTER(ci), C.POINTER(i64), C.POINTER(i64), vp]),
    "vga_hps_files_create": (ci, [vp, ci, C.POINTER(vp)]),
    "vga_hps_files_create_from_infos": (ci, [C.POINTER(vp), C.POINTER(vp), ci, C.POINTER(i64), C.POINTER(vp)]),
    "vga_hps_files_destroy": (None, [vp]),
    "vga_hps_files_totals_of": (ci, [vp, vp]),
    "vga_hps_files_offsets": (ci, [vp, C.POINTER(ci), C.POINTER(i64), C.POINTER(i64)]),
    "vga_hps_files_gc_files": (ci, [vp, vp]),
    "vga_hps_files_ragged": (vp, [vp]),
    "vga_hps_write_device_v": (ci, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "vga_hps_read_device_v": (ci, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "vga_hps_files_write_regions_for": (ci, [vp, ci, vp, i64, C.POINTER(i64)]),
    "vga_hps_files_read_regions_for": (ci, [C.POINTER(vp), C.POINTER(vp), ci, C.POINTER(i64), vp, i64, C.POINTER(i64)]),
    "vga_hps_files_stats": (ci, [vp, C.POINTER(i64)]),
    "vga_hca_decode_device_v": (ci, [vp, vp, vp, vp, C.c_size_t, vp, vp]),
    "vga_hca_encode_device_v": (ci, [vp, vp, vp, vp, vp]),
    "vga_hca_encode_loops_device_v": (ci, [vp, vp, vp, vp, vp]),
    "vga_hca_loop_may_read_tail": (ci, [vp]),
    "vga_testing_hca_encode_v_stats": (ci, [C.POINTER(C.c_longlong), ci]),
    "vga_hca_stream_create": (ci, [vp, vp, C.POINTER(vp)]),
    "vga_hca_stream_encode": (ci, [vp, vp, u8p, C.POINTER(ci)]),
    "vga_hca_stream_pending_frame_count": (ci, [vp]),
    "vga_hca_stream_get_pending_frame": (ci, [vp, u8p]),
    "vga_hca_stream_frames_processed": (ci, [vp]),
    "vga_hca_stream_frame_size": (ci, [vp]),
    "vga_hca_stream_destroy": (None, [vp]),
    "vga_testing_gc_encode_stats": (ci, [C.POINTER(C.c_ulonglong), ci]),
    "vga_testing_gc_plan_pieces": (ci, [ci, ci, ci, C.c_longlong, ci, C.POINTER(ci)]),
    "vga_testing_gc_plan_pieces_n": (ci, [ci, ci, ci, C.c_longlong, ci, ci, C.POINTER(ci)]),
    "vga_set_devices": (ci, [vp, ci]),
    "vga_set_progress_callback": (ci, [vp, vp]),
    "vga_get_devices": (ci, [vp, ci]),
    "vga_testing_hca_frames_per_group_this_thread": (ci, [ci]),
    "vga_dsp_layout_for": (ci, [vp, ci, vp]),
    "vga_dsp_write": (ci, [u8pp, ci, i16p, i16p, i16p, i16p, ci, vp, u8p]),
    "vga_dsp_write_device": (ci, [vp, i64, ci, vp, vp, vp, vp, ci, vp, vp, vp]),
    "vga_nwstm_layout_for": (ci, [vp, ci, vp]),
    "vga_nwstm_write_device": (ci, [vp, ci, ci, vp, vp, i64, ci, vp, vp, vp, vp, vp, i64, ci, vp, i64, vp]),
    "vga_nwstm_write": (ci, [vp, ci, vp, u8pp, ci, i16p, i16p, i16p, i16p, i16pp, ci, u8p]),
    "vga_nwstm_parse": (ci, [u8p, C.c_size_t, vp]),
    "vga_nwstm_read_device": (ci, [vp, vp, i64, ci, vp, i64, vp]),
    "vga_nwstm_read": (ci, [u8p, C.c_size_t, vp, u8pp, i16pp]),
    # include/vgaudio_hip_pcm.h
    "vga_pcm8_encode_device": (ci, [vp, i64, ci, ci, ci, vp, i64, vp]),
    "vga_pcm8_decode_device": (ci, [vp, i64, ci, ci, ci, vp, i64, vp]),
    "vga_nwstm_pcm_layout_for": (ci, [vp, ci, ci, vp]),
    "vga_nwstm_pcm_write_device": (ci, [vp, ci, ci, ci, vp, vp, ci, i64, vp, i64, vp]),
    "vga_nwstm_pcm_write": (ci, [vp, ci, ci, vp, vp, ci, u8p]),
    "vga_nwstm_pcm_parse": (ci, [u8p, C.c_size_t, vp]),
    "vga_nwstm_pcm_read_device": (ci, [vp, vp, i64, ci, vp, ci, i64, vp]),
    "vga_nwstm_pcm_read": (ci, [u8p, C.c_size_t, vp, vp, ci]),
    # include/vgaudio_hip_nwwav.h
    "vga_nwwav_parse": (ci, [u8p, C.c_size_t, vp]),
    "vga_nwwav_read": (ci, [u8p, C.c_size_t, vp, u8pp]),
    "vga_nwwav_bank_create": (ci, [vp, C.POINTER(i64), ci, C.POINTER(vp)]),
    "vga_nwwav_bank_destroy": (None, [vp]),
    "vga_nwwav_bank_channels": (ci, [vp]),
    "vga_nwwav_bank_codec_channels": (ci, [vp, ci]),
    "vga_nwwav_bank_rows": (ci, [vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(i64)]),
    "vga_nwwav_bank_gc_sample_counts": (ci, [vp, C.POINTER(ci)]),
    "vga_nwwav_bank_gc_tables": (ci, [vp, i16p, i16p, i16p, i16p]),
    "vga_nwwav_bank_adpcm_bytes": (i64, [vp]),
    "vga_nwwav_bank_pcm16_samples": (i64, [vp]),
    "vga_nwwav_bank_pcm8_bytes": (i64, [vp]),
    "vga_nwwav_bank_source_bytes": (i64, [vp]),
    "vga_nwwav_bank_read_device": (ci, [vp, vp, vp, vp, vp, vp]),
    "vga_wave_pcm8_file_size": (i64, [vp, ci]),
    "vga_wave_write_pcm8": (ci, [vp, ci, ci, vp, u8p]),
    "vga_wave_write_pcm8_device": (ci, [vp, ci, i64, ci, vp, vp, vp]),
    "vga_wave_read_pcm8": (ci, [u8p, i64, vp, vp, ci]),
    "vga_wave_deinterleave_pcm8_device": (ci, [vp, ci, ci, vp, ci, i64, vp]),
    "vga_hps_layout_for": (ci, [vp, ci, vp]),
    "vga_hps_block_map": (ci, [vp, ci, vp, ci]),
    "vga_hps_write_device": (ci, [vp, ci, ci, vp, i64, ci, vp, vp, vp, vp, i64, ci, vp, i64, vp]),
    "vga_hps_write": (ci, [vp, ci, u8pp, ci, i16p, i16p, i16p, i16pp, ci, u8p]),
    "vga_hps_parse": (ci, [u8p, C.c_size_t, vp, vp, ci]),
    "vga_hps_read_device": (ci, [vp, vp, vp, i64, ci, vp, i64, vp]),
    "vga_hps_read": (ci, [u8p, C.c_size_t, vp, vp, u8pp]),
    "vga_idsp_layout_for": (ci, [vp, ci, vp]),
    "vga_idsp_write_device": (ci, [vp, ci, ci, vp, i64, ci, vp, vp, vp, vp, vp, i64, vp]),
    "vga_idsp_write": (ci, [vp, ci, u8pp, ci, i16p, i16p, i16p, i16p, u8p]),
    "vga_idsp_parse": (ci, [u8p, C.c_size_t, vp]),
    "vga_idsp_read_device": (ci, [vp, vp, i64, ci, vp, i64, vp]),
    "vga_idsp_read": (ci, [u8p, C.c_size_t, vp, u8pp]),
    "vga_genh_parse": (ci, [u8p, C.c_size_t, vp]),
    "vga_genh_read_device": (ci, [vp, vp, i64, ci, vp, i64, vp]),
    "vga_genh_read": (ci, [u8p, C.c_size_t, vp, u8pp]),
    "vga_dsp_parse": (ci, [u8p, C.c_size_t, vp]),
    "vga_dsp_read_device": (ci, [vp, vp, i64, ci, vp, i64, vp]),
    "vga_dsp_read": (ci, [u8p, C.c_size_t, vp, u8pp]),
    "vga_adx_parse": (ci, [u8p, C.c_size_t, vp]),
    "vga_adx_read_device": (ci, [vp, vp, i64, ci, vp, i64, vp]),
    "vga_adx_read": (ci, [u8p, C.c_size_t, vp, u8pp]),
    "vga_hca_parse": (ci, [u8p, C.c_size_t, vp]),
    "vga_hca_read_device": (ci, [vp, vp, i64, ci, vp, i64, vp, vp]),
    "vga_hca_read": (ci, [u8p, C.c_size_t, vp, u8p, C.POINTER(ci)]),
    "vga_testing_adx_read_general_this_thread": (ci, [ci]),
    "vga_testing_adx_last_path_this_thread": (ci, [C.POINTER(ci), C.POINTER(ci)]),
    "vga_gcadpcm_channel_layout_for": (ci, [vp, vp]),
    "vga_gcadpcm_build_channels_batch": (ci, [u8pp, i16p, ci, vp, u8pp, i16pp, i16pp, i16p]),
    "vga_gcadpcm_build_channels_workspace_bytes": (C.c_size_t, [ci, vp]),
    "vga_gcadpcm_build_channels_device": (ci, [vp, i64, vp, ci, vp, vp, i64, vp, i64, vp, i64, vp, vp, C.c_size_t, vp]),
    "vga_adx_default_params": (None, [vp]),
    "vga_adx_calculate_coefficients": (ci, [ci, ci, i16p]),
    "vga_adx_nibble_count_to_sample_count": (ci, [ci, ci]),
    "vga_adx_sample_count_to_nibble_count": (ci, [ci, ci]),
    "vga_adx_sample_count_to_byte_count": (ci, [ci, ci]),
    "vga_adx_encoded_byte_count": (ci, [ci, vp]),
    "vga_adx_encode_batch": (ci, [i16pp, ci, ci, vp, u8pp, i16p]),
    "vga_adx_decode_batch": (ci, [u8pp, ci, ci, ci, vp, i16pp]),
    "vga_adx_encode_batch_v": (ci, [i16pp, C.POINTER(ci), ci, vp, u8pp, i16p]),
    "vga_adx_decode_batch_v": (ci, [u8pp, C.POINTER(ci), ci, C.POINTER(ci), vp, i16pp]),
    "vga_hca_encode_batch_v": (ci, [i16pp, ci, vp, vp, u8pp]),
    "vga_hca_decode_batch_v": (ci, [vp, u8pp, ci, i16pp]),
    "vga_adx_encode_device": (ci, [vp, i64, ci, ci, vp, vp, i64, vp, vp]),
    "vga_adx_decode_device": (ci, [vp, i64, ci, ci, ci, vp, vp, i64, vp, vp]),
    "vga_hca_encoder_initialize": (ci, [vp, vp]),
    "vga_hca_encode_batch": (ci, [i16pp, ci, vp, vp, u8pp]),
    "vga_hca_decode_batch": (ci, [vp, u8pp, ci, i16pp]),
    "vga_hca_decode_workspace_bytes": (C.c_size_t, [vp, ci]),
    "vga_hca_encode_device": (ci, [vp, i64, i64, ci, ci, vp, vp, i64, vp, vp]),
    "vga_hca_decode_device": (ci, [vp, vp, i64, ci, vp, i64, i64, vp, C.c_size_t, vp, vp]),
    # include/vgaudio_hip/adx_files.h
    "vga_adx_files_layout_for": (ci, [vp, ci, C.POINTER(i64), C.POINTER(ci), C.POINTER(i64), C.POINTER(i64), vp]),
    "vga_adx_files_create": (ci, [vp, ci, C.POINTER(i64), C.POINTER(vp)]),
    "vga_adx_files_create_from_infos": (ci, [vp, ci, C.POINTER(i64), C.POINTER(vp)]),
    "vga_adx_files_destroy": (None, [vp]),
    "vga_adx_files_totals_of": (ci, [vp, vp]),
    "vga_adx_files_offsets": (ci, [vp, C.POINTER(ci), C.POINTER(i64), C.POINTER(i64)]),
    "vga_adx_write_device_v": (ci, [vp, vp, vp, vp, vp]),
    "vga_adx_read_device_v": (ci, [vp, vp, vp, vp, vp]),
    "vga_adx_files_write_items_for": (ci, [vp, ci, C.POINTER(i64), ci, vp, i64, C.POINTER(i64)]),
    "vga_adx_files_read_items_for": (ci, [vp, ci, C.POINTER(i64), ci, vp, i64, C.POINTER(i64)]),
    "vga_adx_files_stats": (ci, [vp, C.POINTER(i64)]),
    "vga_adx_files_force_general_this_thread": (ci, [ci]),
    # include/vgaudio_hip_files/wave_files.h
    "vga_wave_files_layout_for": (ci, [vp, ci, C.POINTER(i64), C.POINTER(i64), C.POINTER(ci), C.POINTER(i64), C.POINTER(i64), vp]),
    "vga_wave_files_create": (ci, [vp, ci, C.POINTER(i64), C.POINTER(i64), C.POINTER(vp)]),
    "vga_wave_files_create_from_infos": (ci, [vp, ci, C.POINTER(i64), C.POINTER(i64), C.POINTER(vp)]),
    "vga_wave_files_destroy": (None, [vp]),
    "vga_wave_files_totals_of": (ci, [vp, vp]),
    "vga_wave_files_offsets": (ci, [vp, C.POINTER(ci), C.POINTER(i64), C.POINTER(i64)]),
    "vga_wave_read_device_v": (ci, [vp, vp, vp, vp]),
    "vga_wave_write_device_v": (ci, [vp, vp, vp, vp]),
    "vga_wave_files_write_items_for": (ci, [vp, ci, C.POINTER(i64), C.POINTER(i64), ci, vp, i64, C.POINTER(i64)]),
    "vga_wave_files_read_items_for": (ci, [vp, ci, C.POINTER(i64), C.POINTER(i64), ci, vp, i64, C.POINTER(i64)]),
    "vga_wave_files_stats": (ci, [vp, C.POINTER(i64)]),
    "vga_wave_files_force_general_this_thread": (ci, [ci]),
    # include/vgaudio_hip_files/nw_pcm_files.h
    "vga_nw_pcm_files_layout_for": (ci, [vp, ci, vp, ci, C.POINTER(i64), C.POINTER(i64), C.POINTER(ci), C.POINTER(i64), C.POINTER(i64), vp]),
    "vga_nw_pcm_files_create": (ci, [vp, ci, vp, ci, C.POINTER(i64), C.POINTER(i64), C.POINTER(vp)]),
    "vga_nw_pcm_files_create_from_infos": (ci, [vp, ci, C.POINTER(i64), C.POINTER(i64), C.POINTER(vp)]),
    "vga_nw_pcm_files_destroy": (None, [vp]),
    "vga_nw_pcm_files_totals_of": (ci, [vp, vp]),
    "vga_nw_pcm_files_offsets": (ci, [vp, C.POINTER(ci), C.POINTER(i64), C.POINTER(i64)]),
    "vga_nwstm_pcm_write_device_v": (ci, [vp, vp, vp, vp]),
    "vga_nwstm_pcm_read_device_v": (ci, [vp, vp, vp, vp]),
    "vga_nw_pcm_files_write_items_for": (ci, [vp, ci, vp, ci, C.POINTER(i64), C.POINTER(i64), ci, vp, i64, C.POINTER(i64)]),
    "vga_nw_pcm_files_read_items_for": (ci, [vp, ci, C.POINTER(i64), C.POINTER(i64), ci, vp, i64, C.POINTER(i64)]),
    "vga_nw_pcm_files_stats": (ci, [vp, C.POINTER(i64)]),
    "vga_nw_pcm_files_force_general_this_thread": (ci, [ci]),
    # include/vgaudio_hip/hca_files.h
    "vga_hca_files_layout_for": (ci, [vp, ci, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), vp]),
    "vga_hca_files_create": (ci, [vp, ci, C.POINTER(i64), vp, ci, C.POINTER(vp)]),
    "vga_hca_files_create_from_infos": (ci, [vp, ci, C.POINTER(i64), C.POINTER(ci), vp, ci, C.POINTER(i64), C.POINTER(vp)]),
    "vga_hca_files_destroy": (None, [vp]),
    "vga_hca_files_totals_of": (ci, [vp, vp]),
    "vga_hca_files_offsets": (ci, [vp, C.POINTER(i64), C.POINTER(i64)]),
    "vga_hca_write_device_v": (ci, [vp, vp, vp, vp]),
    "vga_hca_read_device_v": (ci, [vp, vp, vp, vp, vp]),
    "vga_hca_files_write_items_for": (ci, [vp, ci, C.POINTER(i64), ci, vp, i64, C.POINTER(i64)]),
    "vga_hca_files_read_items_for": (ci, [vp, ci, C.POINTER(i64), C.POINTER(i64), ci, vp, i64, C.POINTER(i64)]),
    "vga_hca_files_stats": (ci, [vp, C.POINTER(i64)]),
    "vga_hca_files_force_general_this_thread": (ci, [ci]),
    # include/vgaudio_hip_files/adx_keyed_files.h
    "vga_adx_write_keyed_device_v": (ci, [vp, vp, vp, vp, ci, vp, vp, vp, vp]),
    "vga_adx_read_keyed_device_v": (ci, [vp, vp, vp, ci, vp, vp, vp, vp, vp]),
    "vga_adx_find_keys_workspace_bytes": (C.c_size_t, [vp, ci, ci]),
    "vga_adx_find_keys_device_v": (ci, [vp, vp, vp, ci, ci, vp, vp, C.c_size_t, vp]),
    "vga_adx_find_keys_items_for": (ci, [vp, ci, C.POINTER(i64), vp, i64, C.POINTER(i64)]),
    # include/vgaudio_hip_files/hca_keyed_files.h
    "vga_hca_find_keys_workspace_bytes": (C.c_size_t, [vp, ci]),
    "vga_hca_find_keys_device_v": (ci, [vp, vp, vp, ci, ci, vp, vp, vp, C.c_size_t, vp]),
    "vga_hca_read_keyed_device_v": (ci, [vp, vp, vp, ci, vp, vp, vp, vp, vp]),
    "vga_hca_find_keys_items_for": (ci, [vp, ci, ci, vp, i64, C.POINTER(i64)]),
}


class AdxFileParamsC(C.Structure):
    """vga_adx_file_params"""
    _fields_ = [(n, C.c_int) for n in ("sample_rate", "sample_count", "looping", "loop_start", "loop_end", "alignment_samples",
                                       "frame_size", "version", "type", "highpass_frequency", "encryption_type", "trim_file")]


class AdxFileLayoutC(C.Structure):
    """vga_adx_file_layout"""
    _fields_ = [(n, C.c_int) for n in ("sample_count", "frame_count", "base_header_size", "alignment_bytes", "header_size",
                                       "audio_offset", "audio_size", "footer_offset", "footer_size", "loop_start_offset",
                                       "loop_end_offset", "file_size")]


class AdxFileC(C.Structure):
    """vga_adx_file (include/vgaudio_hip/adx_files.h)"""
    _fields_ = [("channels", C.c_int), ("params", AdxFileParamsC)]


class AdxFilesTotalsC(C.Structure):
    """vga_adx_files_totals"""
    _fields_ = [("files", C.c_int), ("channels", C.c_int), ("audio_bytes", C.c_int64), ("image_bytes", C.c_int64)]


class AdxFilesItemC(C.Structure):
    """vga_adx_files_item"""
    _fields_ = [("form", C.c_int), ("file", C.c_int), ("x", C.c_int), ("y", C.c_uint32), ("granule", C.c_int),
                ("begin", C.c_int64), ("end", C.c_int64), ("keep_end", C.c_int64)]


class AdxFindKeysItemC(C.Structure):
    """vga_adx_find_keys_item (include/vgaudio_hip_files/adx_keyed_files.h)"""
    _fields_ = [("file", C.c_int), ("first_slot", C.c_int), ("slot_count", C.c_int)]


class HcaFindKeysItemC(C.Structure):
    """vga_hca_find_keys_item (include/vgaudio_hip_files/hca_keyed_files.h)"""
    _fields_ = [("file", C.c_int), ("first_key", C.c_int), ("key_count", C.c_int)]


class WaveInfoC(C.Structure):
    """vga_wave_info"""
    _fields_ = ([(n, C.c_int) for n in ("channel_count", "sample_rate", "bits_per_sample", "sample_count", "sample_count_declared",
                                        "looping", "loop_start", "loop_end")]
                + [("data_offset", C.c_int64), ("data_size", C.c_int), ("data_size_declared", C.c_int)])


class WaveParamsC(C.Structure):
    """vga_wave_params"""
    _fields_ = [(n, C.c_int) for n in ("sample_rate", "sample_count", "looping", "loop_start", "loop_end")]


class WaveFileC(C.Structure):
    """vga_wave_file (include/vgaudio_hip_files/wave_files.h)"""
    _fields_ = [("channels", C.c_int), ("bits", C.c_int), ("params", WaveParamsC)]


class WaveFilesTotalsC(C.Structure):
    """vga_wave_files_totals"""
    _fields_ = [("files", C.c_int), ("channels", C.c_int), ("pcm_samples", C.c_int64), ("image_bytes", C.c_int64)]


class WaveFilesItemC(C.Structure):
    """vga_wave_files_item"""
    _fields_ = [("form", C.c_int), ("file", C.c_int), ("x", C.c_int), ("y", C.c_uint32), ("span", C.c_int),
                ("begin", C.c_int64), ("end", C.c_int64)]


class AdxKeyC(C.Structure):
    """vga_adx_key"""
    _fields_ = [("seed", C.c_int), ("mult", C.c_int), ("inc", C.c_int)]


class DspParamsC(C.Structure):
    """vga_dsp_params"""
    _fields_ = [(n, C.c_int) for n in ("sample_rate", "sample_count", "looping", "loop_start", "loop_end",
                                       "samples_per_interleave", "loop_point_alignment", "trim_file")]


class DspLayoutC(C.Structure):
    """vga_dsp_layout"""
    _fields_ = [(n, C.c_int) for n in ("sample_count", "loop_start", "loop_end", "start_addr", "end_addr", "cur_addr",
                                       "bytes_per_interleave", "frames_per_interleave", "audio_data_size", "file_size")]


class GcChannelParamsC(C.Structure):
    """vga_gcadpcm_channel_params (include/vgaudio_hip.h)"""
    _fields_ = [(n, C.c_int) for n in ("sample_count", "looping", "loop_start", "loop_end", "loop_alignment_multiple",
                                       "samples_per_seek_table_entry")]


class GcChannelLayoutC(C.Structure):
    """vga_gcadpcm_channel_layout"""
    _fields_ = [(n, C.c_int) for n in ("alignment_needed", "loop_start_aligned", "sample_count_aligned",
                                       "seek_table_entries")]


class GcFileC(C.Structure):
    """vga_gc_file (include/vgaudio_hip/gc_files.h)"""
    _fields_ = [("channels", C.c_int), ("sample_rate", C.c_int), ("channel", GcChannelParamsC)]


class DspFileConfigC(C.Structure):
    """vga_dsp_file_config"""
    _fields_ = [(n, C.c_int) for n in ("samples_per_interleave", "loop_point_alignment", "trim_file")]


class GcFilesTotalsC(C.Structure):
    """vga_gc_files_totals"""
    _fields_ = [("files", C.c_int), ("channels", C.c_int), ("pcm_samples", C.c_int64), ("adpcm_bytes", C.c_int64),
                ("seek_shorts", C.c_int64), ("image_bytes", C.c_int64), ("build_workspace_bytes", C.c_size_t)]


class GcAlignedTotalsC(C.Structure):
    """vga_gc_aligned_totals (include/vgaudio_hip/gc_files_aligned.h)"""
    _fields_ = [("files", C.c_int), ("channels", C.c_int), ("aligned_channels", C.c_int), ("pcm_samples", C.c_int64),
                ("adpcm_bytes", C.c_int64), ("out_pcm_samples", C.c_int64), ("out_adpcm_bytes", C.c_int64), ("seek_shorts", C.c_int64),
                ("workspace_bytes", C.c_size_t)]


NW_MAX_CHANNELS = NW_MAX_TRACKS = 255


class NwTrackC(C.Structure):
    """vga_nw_track"""
    _fields_ = [(n, C.c_int) for n in ("channel_count", "left", "right", "volume", "panning")]


class NwParamsC(C.Structure):
    """vga_nwstm_params"""
    _fields_ = ([(n, C.c_int) for n in ("target", "sample_rate", "sample_count", "looping", "loop_start", "loop_end",
                                        "samples_per_interleave", "samples_per_seek_table_entry", "loop_point_alignment",
                                        "track_type", "seek_table_type")]
                + [("version", C.c_uint32)]
                + [(n, C.c_int) for n in ("endianness", "track_count", "keep_seek_table", "keep_loop_context")])


class NwLayoutC(C.Structure):
    """vga_nwstm_layout"""
    _fields_ = ([("target", C.c_int), ("endianness", C.c_int), ("version", C.c_uint32)]
                + [(n, C.c_int) for n in ("include_track_info", "include_region_info", "include_unaligned_loop",
                                          "version_word", "looping", "loop_start", "loop_end", "sample_count",
                                          "alignment_needed")]
                + [("channel", GcChannelParamsC)]
                + [(n, C.c_int) for n in (
                    "channel_sample_count", "channel_adpcm_bytes", "channel_seek_entries", "samples_per_interleave",
                    "interleave_size", "interleave_count", "last_block_samples", "last_block_size_without_padding",
                    "last_block_size", "samples_per_seek_table_entry", "bytes_per_seek_table_entry",
                    "seek_table_entry_count", "track_count", "header_size", "head_block_offset", "head_block_size",
                    "head1_size", "head2_size", "head3_size", "seek_block_offset", "seek_block_size",
                    "data_block_offset", "data_block_size", "audio_data_offset", "audio_data_size", "file_size")])


class NwInfoC(C.Structure):
    """vga_nwstm_info"""
    _fields_ = ([("target", C.c_int), ("endianness", C.c_int), ("version", C.c_uint32)]
                + [(n, C.c_int) for n in (
                    "codec", "looping", "loop_start", "sample_count", "sample_rate", "channel_count", "has_unaligned_loop",
                    "loop_start_unaligned", "loop_end_unaligned", "interleave_count", "interleave_size",
                    "samples_per_interleave", "last_block_size_without_padding", "last_block_samples", "last_block_size",
                    "bytes_per_seek_table_entry", "samples_per_seek_table_entry", "track_type", "seek_table_type",
                    "has_track_info", "track_count")]
                + [("tracks", NwTrackC * NW_MAX_TRACKS), ("coefs", (C.c_int16 * 16) * NW_MAX_CHANNELS),
                   ("gain", C.c_int16 * NW_MAX_CHANNELS), ("start_context", (C.c_int16 * 3) * NW_MAX_CHANNELS),
                   ("loop_context", (C.c_int16 * 3) * NW_MAX_CHANNELS)]
                + [(n, C.c_int) for n in (
                    "seek_table_offset", "seek_entries", "seek_big_endian", "head_block_offset", "head_block_size",
                    "seek_block_offset", "seek_block_size", "data_block_offset", "data_block_size", "audio_data_offset",
                    "audio_data_length", "adpcm_bytes", "file_size")])


class NwFileC(C.Structure):
    """vga_nw_file (include/vgaudio_hip/nw_files.h)"""
    _fields_ = [(n, C.c_int) for n in ("channels", "sample_rate", "sample_count", "looping", "loop_start", "loop_end")]


class NwFileConfigC(C.Structure):
    """vga_nw_file_config"""
    _fields_ = ([(n, C.c_int) for n in ("target", "samples_per_interleave", "samples_per_seek_table_entry", "loop_point_alignment",
                                        "track_type", "seek_table_type")]
                + [("version", C.c_uint32), ("endianness", C.c_int)])


class NwFilesTotalsC(C.Structure):
    """vga_nw_files_totals"""
    _fields_ = [("files", C.c_int), ("channels", C.c_int), ("pcm_samples", C.c_int64), ("adpcm_bytes", C.c_int64),
                ("seek_shorts", C.c_int64), ("image_bytes", C.c_int64)]


class NwPcmFilesTotalsC(C.Structure):
    """vga_nw_pcm_files_totals (include/vgaudio_hip_files/nw_pcm_files.h)"""
    _fields_ = [("files", C.c_int), ("channels", C.c_int), ("pcm_samples", C.c_int64), ("image_bytes", C.c_int64)]


class NwPcmFilesItemC(C.Structure):
    """vga_nw_pcm_files_item"""
    _fields_ = [("form", C.c_int), ("file", C.c_int), ("x", C.c_int), ("y", C.c_uint32), ("conv", C.c_int),
                ("begin", C.c_int64), ("end", C.c_int64)]


class NwWavInfoC(C.Structure):
    """vga_nwwav_info"""
    _fields_ = ([("kind", C.c_int), ("endianness", C.c_int), ("version", C.c_uint32)]
                + [(n, C.c_int) for n in (
                    "file_size", "codec", "looping", "loop_start", "sample_count", "sample_rate", "channel_count",
                    "channel_bytes", "has_loop_start_unaligned", "loop_start_unaligned", "prefetch_count",
                    "prefetch_start_sample", "prefetch_size", "prefetch_audio_offset", "stream_looping",
                    "stream_sample_count", "interleave_count", "interleave_size", "samples_per_interleave",
                    "last_block_size_without_padding", "last_block_samples", "last_block_size")]
                + [("audio_offset", C.c_int * NW_MAX_CHANNELS), ("coefs", (C.c_int16 * 16) * NW_MAX_CHANNELS),
                   ("gain", C.c_int16 * NW_MAX_CHANNELS), ("start_context", (C.c_int16 * 3) * NW_MAX_CHANNELS),
                   ("loop_context", (C.c_int16 * 3) * NW_MAX_CHANNELS)])


GC_CONTAINER_MAX_CHANNELS = 255
_GCM = GC_CONTAINER_MAX_CHANNELS


class HpsParamsC(C.Structure):
    """vga_hps_params"""
    _fields_ = [(n, C.c_int) for n in ("sample_rate", "sample_count", "looping", "loop_start", "loop_end")]


class HpsLayoutC(C.Structure):
    """vga_hps_layout"""
    _fields_ = ([(n, C.c_int) for n in ("header_size", "channel_size", "alignment", "alignment_needed")]
                + [("channel", GcChannelParamsC)]
                + [(n, C.c_int) for n in ("sample_count", "looping", "loop_start", "loop_end", "channel_adpcm_bytes",
                                          "block_header_size", "block_count", "loop_block", "file_size")])


class HpsBlockC(C.Structure):
    """vga_hps_block"""
    _fields_ = [(n, C.c_int) for n in ("offset", "next_offset", "start_sample", "byte_in_index", "channel_size", "written_size",
                                       "total_size", "end_nibble")]


class HpsInfoC(C.Structure):
    """vga_hps_info"""
    _fields_ = ([(n, C.c_int) for n in ("sample_rate", "channel_count", "sample_count", "looping", "loop_start")]
                + [("max_block_size", C.c_int * _GCM), ("end_address", C.c_int * _GCM), ("coefs", (C.c_int16 * 16) * _GCM),
                   ("gain", C.c_int16 * _GCM), ("start_context", (C.c_int16 * 3) * _GCM),
                   ("loop_context", (C.c_int16 * 3) * _GCM)]
                + [(n, C.c_int) for n in ("block_count", "adpcm_bytes")])


class HpsBlockInfoC(C.Structure):
    """vga_hps_block_info"""
    _fields_ = [(n, C.c_int) for n in ("offset", "next_offset", "size", "final_nibble", "audio_offset", "audio_bytes",
                                       "out_offset")]


class IdspParamsC(C.Structure):
    """vga_idsp_params"""
    _fields_ = [(n, C.c_int) for n in ("sample_rate", "sample_count", "looping", "loop_start", "loop_end", "block_size",
                                       "trim_file")]


class IdspLayoutC(C.Structure):
    """vga_idsp_layout"""
    _fields_ = ([("alignment_needed", C.c_int), ("channel", GcChannelParamsC)]
                + [(n, C.c_int) for n in ("channel_sample_count", "channel_adpcm_bytes", "sample_count", "looping", "loop_start",
                                          "loop_end", "start_addr", "end_addr", "cur_addr", "interleave_size", "header_size",
                                          "audio_data_size", "file_size")])


class IdspInfoC(C.Structure):
    """vga_idsp_info"""
    _fields_ = ([(n, C.c_int) for n in ("channel_count", "sample_rate", "sample_count", "loop_start", "loop_end",
                                        "interleave_size", "header_size", "channel_info_size", "audio_data_offset",
                                        "audio_data_length", "looping")]
                + [("channel_sample_count", C.c_int * _GCM), ("channel_looping", C.c_int * _GCM),
                   ("start_address", C.c_int * _GCM), ("end_address", C.c_int * _GCM), ("coefs", (C.c_int16 * 16) * _GCM),
                   ("gain", C.c_int16 * _GCM), ("start_context", (C.c_int16 * 3) * _GCM),
                   ("loop_context", (C.c_int16 * 3) * _GCM)]
                + [(n, C.c_int) for n in ("interleave", "adpcm_bytes")])


class IdspFileC(C.Structure):
    """vga_idsp_file (include/vgaudio_hip_files/idsp_files.h)"""
    _fields_ = [(n, C.c_int) for n in ("channels", "sample_rate", "sample_count", "looping", "loop_start", "loop_end")]


class IdspFileConfigC(C.Structure):
    """vga_idsp_file_config"""
    _fields_ = [("block_size", C.c_int), ("trim_file", C.c_int)]


class IdspFilesTotalsC(C.Structure):
    """vga_idsp_files_totals"""
    _fields_ = [("files", C.c_int), ("channels", C.c_int), ("pcm_samples", C.c_int64), ("adpcm_bytes", C.c_int64),
                ("image_bytes", C.c_int64)]


class IdspFilesRegionC(C.Structure):
    """vga_idsp_files_region"""
    _fields_ = [("kernel", C.c_int), ("index", C.c_int), ("granule", C.c_int), ("begin", C.c_int64), ("end", C.c_int64)]


class HpsFileC(C.Structure):
    """vga_hps_file (include/vgaudio_hip_files/hps_files.h)"""
    _fields_ = [(n, C.c_int) for n in ("channels", "sample_rate", "sample_count", "looping", "loop_start", "loop_end")]


class HpsFilesTotalsC(C.Structure):
    """vga_hps_files_totals"""
    _fields_ = [("files", C.c_int), ("channels", C.c_int), ("pcm_samples", C.c_int64), ("adpcm_bytes", C.c_int64),
                ("image_bytes", C.c_int64), ("blocks", C.c_int64)]


class HpsFilesRegionC(C.Structure):
    """vga_hps_files_region"""
    _fields_ = [("kernel", C.c_int), ("index", C.c_int), ("granule", C.c_int), ("begin", C.c_int64), ("end", C.c_int64)]


class GenhInfoC(C.Structure):
    """vga_genh_info"""
    _fields_ = ([(n, C.c_int) for n in ("channel_count", "interleave", "sample_rate", "loop_start", "loop_end", "codec",
                                        "audio_data_offset", "header_size")]
                + [("coef_offset", C.c_int * 2), ("interleave_type", C.c_int), ("coef_type", C.c_int),
                   ("coef_split_offset", C.c_int * 2), ("sample_count", C.c_int), ("looping", C.c_int),
                   ("coefs", (C.c_int16 * 16) * 2), ("adpcm_bytes", C.c_int)])


class HcaInfoC(C.Structure):
    """vga_hca_info (include/vgaudio_hip.h) == HcaInfo."""
    _fields_ = [(n, C.c_int) for n in (
        "channel_count", "sample_rate", "sample_count", "frame_count", "inserted_samples", "appended_samples",
        "header_size", "frame_size", "min_resolution", "max_resolution", "track_count", "channel_config",
        "total_band_count", "base_band_count", "stereo_band_count", "hfr_band_count", "bands_per_hfr_group",
        "hfr_group_count", "looping", "loop_start_frame", "loop_end_frame", "pre_loop_samples", "post_loop_samples",
        "use_ath_curve", "comment_length")]


DSP_MAX_CHANNELS = 255


class DspInfoC(C.Structure):
    """vga_dsp_info"""
    _fields_ = ([(n, C.c_int) for n in ("sample_count", "nibble_count", "sample_rate", "looping", "format", "start_addr",
                                        "end_addr", "cur_addr", "channel_count", "frames_per_interleave", "loop_start",
                                        "loop_end")]
                + [("coefs", (C.c_int16 * 16) * DSP_MAX_CHANNELS), ("gain", C.c_int16 * DSP_MAX_CHANNELS),
                   ("start_context", (C.c_int16 * 3) * DSP_MAX_CHANNELS), ("loop_context", (C.c_int16 * 3) * DSP_MAX_CHANNELS)]
                + [(n, C.c_int) for n in ("audio_offset", "adpcm_bytes", "interleave_size", "data_length")])


class AdxFileInfoC(C.Structure):
    """vga_adx_file_info"""
    _fields_ = ([(n, C.c_int) for n in ("header_size", "type", "frame_size", "bit_depth", "channel_count", "sample_rate",
                                        "sample_count", "highpass_frequency", "version", "revision", "inserted_samples",
                                        "loop_count", "looping", "loop_type", "loop_start_sample", "loop_start_byte",
                                        "loop_end_sample", "loop_end_byte")]
                + [("history", (C.c_int16 * 2) * 255)]
                + [(n, C.c_int) for n in ("audio_offset", "samples_per_frame", "frame_count", "audio_bytes")])


class HcaFileInfoC(C.Structure):
    """vga_hca_file_info"""
    _fields_ = ([("hca", HcaInfoC), ("version", C.c_int), ("encryption_type", C.c_int), ("volume", C.c_float)]
                + [(n, C.c_int) for n in ("vbr_max_frame_size", "vbr_noise_level", "dec_stereo_type", "reserved1", "reserved2",
                                          "has_ath_chunk", "has_comment")]
                + [("comment", C.c_char * 256), ("frames_offset", C.c_int)])


class HcaFileC(C.Structure):
    """vga_hca_file (include/vgaudio_hip/hca_files.h)"""
    _fields_ = [("hca", HcaInfoC), ("comment", C.c_char_p), ("volume", C.c_float), ("encryption_type", C.c_int),
                ("encrypted_ids", C.c_int), ("key", C.c_int)]


class HcaFilesTotalsC(C.Structure):
    """vga_hca_files_totals"""
    _fields_ = [("files", C.c_int), ("total_frames", C.c_int64), ("frame_bytes", C.c_int64), ("image_bytes", C.c_int64)]


class HcaFilesItemC(C.Structure):
    """vga_hca_files_item"""
    _fields_ = [("form", C.c_int), ("file", C.c_int), ("first_frame", C.c_int), ("frames", C.c_int), ("begin", C.c_int64),
                ("end", C.c_int64)]


class HcaParamsC(C.Structure):
    """vga_hca_params == CriHcaParameters."""
    _fields_ = [(n, C.c_int) for n in ("quality", "bitrate", "limit_bitrate", "channel_count", "sample_rate",
                                       "sample_count", "looping", "loop_start", "loop_end")]


class AdxParams(C.Structure):
    """vga_adx_params (include/vgaudio_hip.h) == CriAdxParameters."""
    _fields_ = [("sample_rate", C.c_int), ("highpass_frequency", C.c_int), ("frame_size", C.c_int),
                ("version", C.c_int), ("history", C.c_int16), ("padding", C.c_int), ("type", C.c_int),
                ("filter", C.c_int)]


def _preload_torch_hip_runtime():
    """One HIP runtime per process: PyTorch wheels bundle their own libamdhip64 (SONAME
    libamdhip64.so.7, same as /opt/rocm's).  If this library were loaded first it would bind
    /opt/rocm's copy, torch would then load its own, and the second HSA runtime in the process
    reports "no ROCm-capable device".  Pre-loading torch's copy (when torch is installed) makes
    both resolve to the same runtime regardless of import order.  Without torch (C#/C++ hosts)
    the system ROCm runtime is used."""
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def lib():
    """Load the shared library (built in-tree by `python -m vgaudio_amd.build`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise OSError(f"{SO_PATH} not found: run `python -m vgaudio_amd.build` (hipcc, gfx950). "
                          "There is no CPU fallback.")
        _preload_torch_hip_runtime()
        L = C.CDLL(SO_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _lib = L
    return _lib


def check(rc):
    if rc == VGA_OK:
        return
    msg = lib().vga_last_error().decode("utf-8", "replace")
    raise _EXC.get(rc, VgaError)(msg or f"vgaudio_hip error {rc}")

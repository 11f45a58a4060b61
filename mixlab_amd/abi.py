"""ctypes binding of include/mixlab_gpu.h (plumbing for tests and bench.py -- the product is the .so).

There is no CPU fallback: if libmixlab_gpu.so is missing this module raises at import.
"""
from __future__ import annotations

import ctypes as C
import pathlib

import numpy as np

_PKG = pathlib.Path(__file__).resolve().parent
LIB_PATH = _PKG / "libmixlab_gpu.so"

if not LIB_PATH.exists():
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -m mixlab_amd.build` (hipcc, gfx950). "
        "mixlab_amd has no CPU fallback."
    )

lib = C.CDLL(str(LIB_PATH))

# ---- constants (include/mixlab_gpu.h) ----
MX_OK, MX_ERR_INVALID, MX_ERR_TYPE, MX_ERR_DEVICE, MX_ERR_NOMEM, MX_ERR_INTERNAL, MX_ERR_FULL = 0, -1, -2, -3, -4, -5, -6
MX_DISCONNECTED, MX_MONO, MX_STEREO, MX_VIDEO = 0, 1, 2, 3
(KIND_AMPLIFIER, KIND_ENVELOPE, KIND_EQ_THREE, KIND_FM_SINE, KIND_MIXER, KIND_OSCILLATOR, KIND_PLOTTER,
 KIND_STEREO_PANNER, KIND_STEREO_SPLITTER, KIND_TRIGGER, KIND_VIDEO_MIXER, KIND_SOURCE_MONO,
 KIND_SOURCE_STEREO, KIND_SOURCE_VIDEO, KIND_VIDEO_TO_RGBA, KIND_FIR, KIND_RESAMPLE, KIND_MONITOR, KIND_OUTPUT_DEVICE, KIND_COUNT) = range(20)
PROFILE_KINDS = 18   # MX_PROFILE_KINDS: floats mx_graph_profile_run / _collect write (an OutputDevice's time is in ms_total)
KIND_NAMES = ["amplifier", "envelope", "eq_three", "fm_sine", "mixer", "oscillator", "plotter", "stereo_panner",
              "stereo_splitter", "trigger", "video_mixer", "source_mono", "source_stereo", "source_video", "video_to_rgba", "fir", "resample", "monitor",
              "output_device"]
WAVE_ON, WAVE_OFF, WAVE_SINE, WAVE_SQUARE, WAVE_TRIANGLE, WAVE_SAW = range(6)
FLAG_EQ_EXACT = 1   # the default (kept as a no-op name)
FLAG_NO_FUSE = 2
FLAG_EQ_FAST = 4    # time-parallel EqThree: <= 1 ULP, not bit-exact
FLAG_FP_CONTRACT = 16   # the contracted order (mul+add fused): <= 1 ULP of the exact order, equal to the oracle's contract mode
FLAG_OVERLAP_TAIL = 8   # the last Mixer bank runs on a second stream beside the next run's earlier groups
# MX_EQ_LAUNCH_* (mx_graph_debug_eq_launch): the form an EqThree launch took
EQ_LAUNCH = {0: "none", 1: "sequential", 2: "direct", 3: "tiled", 4: "ragged_tick", 5: "control_tile", 6: "scan"}


class MixerChannelParams(C.Structure):
    _fields_ = [("gain_db", C.c_double), ("fader", C.c_double), ("cue", C.c_uint8), ("_pad", C.c_uint8 * 7)]


class EqThreeParams(C.Structure):
    _fields_ = [("gain_lo_db", C.c_double), ("gain_mid_db", C.c_double), ("gain_hi_db", C.c_double)]


class EnvelopeParams(C.Structure):
    _fields_ = [("attack_ms", C.c_double), ("decay_ms", C.c_double), ("sustain_amplitude", C.c_double), ("release_ms", C.c_double)]


class AmplifierParams(C.Structure):
    _fields_ = [("amplitude", C.c_double), ("mod_depth", C.c_double)]


class OscillatorParams(C.Structure):
    _fields_ = [("freq", C.c_double), ("waveform", C.c_uint32), ("_pad", C.c_uint32)]


class FmSineParams(C.Structure):
    _fields_ = [("freq_lo", C.c_double), ("freq_hi", C.c_double)]


class TriggerParams(C.Structure):
    _fields_ = [("gate_open", C.c_uint32)]


class Node(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("params_len", C.c_uint32), ("params", C.c_void_p)]


class Edge(C.Structure):
    _fields_ = [("src_node", C.c_uint32), ("src_port", C.c_uint32), ("dst_node", C.c_uint32), ("dst_port", C.c_uint32)]


class GraphOpts(C.Structure):
    _fields_ = [("sample_rate", C.c_uint32), ("ticks_per_second", C.c_uint32), ("max_ticks_per_run", C.c_uint32),
                ("flags", C.c_uint32), ("device", C.c_int32), ("_pad", C.c_int32), ("stream", C.c_void_p)]


class Frame(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("data", C.c_void_p * 3), ("stride", C.c_int32 * 3),
                ("dur_num", C.c_int64), ("dur_den", C.c_int64), ("off_num", C.c_int64), ("off_den", C.c_int64)]


class Input(C.Structure):
    _fields_ = [("kind", C.c_int), ("samples", C.c_void_p), ("len", C.c_size_t), ("video", C.c_void_p)]


class Output(C.Structure):
    _fields_ = [("kind", C.c_int), ("samples", C.c_void_p), ("len", C.c_size_t), ("video", C.c_void_p), ("video_present", C.c_int)]


def _proto(name, restype, *argtypes):
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = list(argtypes)
    return fn


_proto("mx_last_error", C.c_char_p)
_proto("mx_abi_version", C.c_uint32)
_proto("mx_device_count", C.c_int)
_proto("mx_graph_build", C.c_int, C.POINTER(Node), C.c_size_t, C.POINTER(Edge), C.c_size_t, C.POINTER(GraphOpts), C.POINTER(C.c_void_p))
_proto("mx_graph_destroy", None, C.c_void_p)
_proto("mx_graph_samples_per_tick", C.c_int, C.c_void_p, C.POINTER(C.c_size_t))
_proto("mx_graph_run_order", C.c_int, C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t))
_proto("mx_graph_update_params", C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t)
class ParamEvent(C.Structure):
    """mx_param_event: ModuleT::update of `node` at the boundary before tick `tick_in_run` of the next run."""
    _fields_ = [("node", C.c_uint32), ("tick_in_run", C.c_uint32), ("params", C.c_void_p), ("params_len", C.c_size_t)]


_proto("mx_graph_schedule_params", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t)
_proto("mx_graph_schedule_params_batch", C.c_int, C.c_void_p, C.POINTER(ParamEvent), C.c_size_t)
_proto("mx_graph_eq_spec_stats", C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
_proto("mx_graph_debug_eq_records", C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t))
_proto("mx_graph_debug_tail_releases", C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
_proto("mx_graph_debug_eq_launch", C.c_int, C.c_void_p, C.POINTER(C.c_uint32))
_proto("mx_graph_debug_eq_env_rows", C.c_int, C.c_void_p, C.POINTER(C.c_uint32))
_proto("mx_graph_debug_eq_lean", C.c_int, C.c_void_p, C.POINTER(C.c_uint32))
_proto("mx_graph_eq_repair_stats", C.c_int, C.c_void_p, C.POINTER(C.c_uint64))
PLAN_NONE = 2**64 - 1   # mx_plan_node.out_off / out_off2: no buffer


class PlanNode(C.Structure):
    """mx_plan_node: what the graph compiler says about one node (mx_graph_debug_plan)."""
    _fields_ = [("pos", C.c_int32), ("level", C.c_int32), ("group", C.c_int32), ("slot", C.c_uint32), ("sub_key", C.c_int32),
                ("dom_num", C.c_uint32), ("dom_den", C.c_uint32), ("in_dom_num", C.c_uint32), ("in_dom_den", C.c_uint32),
                ("elided", C.c_uint32), ("owner", C.c_int32),
                ("fuse_pan", C.c_int32), ("fuse_amp", C.c_int32), ("fuse_trigger", C.c_int32), ("fuse_env", C.c_int32),
                ("n_out", C.c_uint32), ("out_elided", C.c_uint8 * 4), ("out_dup", C.c_uint8 * 4),
                ("out_off", C.c_uint64 * 4), ("out_off2", C.c_uint64 * 4)]


class PlanInfo(C.Structure):
    """mx_plan_info: the plan as a whole (mx_graph_debug_plan)."""
    _fields_ = [("n_order", C.c_uint64), ("n_groups", C.c_uint64), ("slab_floats", C.c_uint64), ("zero_off", C.c_uint64), ("zero_floats", C.c_uint64),
                ("tail_first_group", C.c_int32), ("tail_ports", C.c_uint32), ("tail_auto", C.c_uint32), ("has_video", C.c_uint32)]


_proto("mx_graph_debug_plan", C.c_int, C.POINTER(Node), C.c_size_t, C.POINTER(Edge), C.c_size_t, C.POINTER(GraphOpts), C.c_uint32, C.c_size_t,
       C.POINTER(PlanNode), C.POINTER(PlanInfo))
_proto("mx_graph_write_source", C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t)
_proto("mx_graph_bind_source_device", C.c_int, C.c_void_p, C.c_uint32, C.c_void_p)
_proto("mx_graph_run_ticks", C.c_int, C.c_void_p, C.c_uint64, C.c_uint32)
_proto("mx_graph_sync", C.c_int, C.c_void_p)
_proto("mx_graph_read_output", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t)
_proto("mx_graph_read_output_window", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_size_t)
_proto("mx_graph_read_output_i16", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t)
_proto("mx_graph_write_source_i16", C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t)
_proto("mx_graph_output_device_ptr", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t))
_proto("mx_graph_tail_stream", C.c_int, C.c_void_p, C.POINTER(C.c_void_p))
_proto("mx_graph_stream", C.c_int, C.c_void_p, C.POINTER(C.c_void_p))
_proto("mx_graph_read_plotter", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int))
class OutputDeviceParams(C.Structure):
    """mx_output_device_params: channels of the open stream (0 = none), left / right (-1 = None)."""
    _fields_ = [("channels", C.c_uint32), ("left", C.c_int32), ("right", C.c_int32), ("_pad", C.c_uint32)]


class AudioOutTick(C.Structure):
    """mx_audio_out_tick: one tick's clip bit, Clip / Lag statuses (0 None, 1 Recent, 2 Active), changed, channels."""
    _fields_ = [("clip", C.c_uint8), ("clip_status", C.c_uint8), ("lag_status", C.c_uint8), ("changed", C.c_uint8), ("channels", C.c_uint32)]


AUDIO_OUT_TICK_DTYPE = np.dtype([("clip", np.uint8), ("clip_status", np.uint8), ("lag_status", np.uint8), ("changed", np.uint8), ("channels", np.uint32)])
_proto("mx_graph_read_audio_out", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t))
_proto("mx_graph_audio_out_lag", C.c_int, C.c_void_p, C.c_uint32)
class PortRef(C.Structure):
    """mx_port_ref: an output terminal (node, port) a meter taps."""
    _fields_ = [("node", C.c_uint32), ("port", C.c_uint32)]


class MeterParams(C.Structure):
    """mx_meter_params: ticks a peak is held before it decays, and the per-tick decay factor (finite, 0 < release <= 1)."""
    _fields_ = [("hold_ticks", C.c_uint32), ("release", C.c_float)]


METER_TICK_DTYPE = np.dtype({"names": ["peak", "hold", "sum_sq", "over", "frames", "channels"],
                             "formats": [(np.float32, 2), (np.float32, 2), (np.float64, 2), (np.uint32, 2), np.uint32, np.uint32],
                             "offsets": [0, 8, 16, 32, 40, 44], "itemsize": 48})   # mx_meter_tick
_proto("mx_graph_set_meters", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
_proto("mx_graph_read_meters", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t)
class SpectrumParams(C.Structure):
    """mx_spectrum_params: one transform size and band layout for every spectrum tap of a graph."""
    _fields_ = [("n_fft", C.c_uint32), ("n_bands", C.c_uint32), ("edges", C.POINTER(C.c_uint16))]


_proto("mx_graph_set_spectra", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
_proto("mx_graph_read_spectra", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t)
_proto("mx_spectrum_tables", C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
class LoudnessParams(C.Structure):
    """mx_loudness_params: the momentary and the short-term window in ticks (1 .. 1024 each; 24 and 180 are 400 ms and 3 s at 60 ticks/s)."""
    _fields_ = [("momentary_ticks", C.c_uint32), ("short_ticks", C.c_uint32)]


LOUDNESS_TICK_DTYPE = np.dtype({"names": ["ksq", "momentary_sq", "short_sq", "true_peak", "frames", "channels"],
                                "formats": [(np.float64, 2), np.float64, np.float64, (np.float32, 2), np.uint32, np.uint32],
                                "offsets": [0, 16, 24, 32, 40, 44], "itemsize": 48})   # mx_loudness_tick
_proto("mx_graph_set_loudness", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
_proto("mx_graph_read_loudness", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t)
_proto("mx_loudness_tables", C.c_int, C.c_double, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_proto("mx_loudness_gate", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_size_t))
class StereoParams(C.Structure):
    """mx_stereo_params: the window in ticks (1 .. 1024), the goniometer's grid (0: none, 64, 128), its zoom (0 .. 8) and emission period."""
    _fields_ = [("window_ticks", C.c_uint32), ("grid", C.c_uint32), ("zoom_log2", C.c_uint32), ("hop", C.c_uint32)]


STEREO_TICK_DTYPE = np.dtype({"names": ["sum_ll", "sum_rr", "sum_lr", "win_ll", "win_rr", "win_lr", "frames", "nonfinite"],
                              "formats": [np.float64] * 6 + [np.uint32] * 2,
                              "offsets": [0, 8, 16, 24, 32, 40, 48, 52], "itemsize": 56})   # mx_stereo_tick
_proto("mx_graph_set_stereo", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
_proto("mx_graph_read_stereo", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t)
_proto("mx_graph_read_goniometers", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32))
_proto("mx_stereo_gonio_record_bytes", C.c_int, C.POINTER(StereoParams), C.POINTER(C.c_size_t))
_proto("mx_stereo_correlation", C.c_int, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double))
class LimiterParams(C.Structure):
    """mx_limiter_params: the ceiling (finite, 2^-20 .. 1) and the lookahead in frames of the port's own rate (0 .. 512)."""
    _fields_ = [("ceiling", C.c_float), ("lookahead", C.c_uint32)]


LIMITER_MAX_LOOKAHEAD = 512   # MX_LIMITER_MAX_LOOKAHEAD
LIMITER_TILE = 2048           # frames of a run one workgroup of the limiter kernel limits (mx_kernels.hpp LIMIT_TILE): tests put peaks on its edges
LIMITER_TICK_DTYPE = np.dtype({"names": ["min_gain", "peak_out", "limited", "nonfinite", "frames", "channels"],
                               "formats": [np.float32, np.float32, np.uint32, np.uint32, np.uint32, np.uint32],
                               "offsets": [0, 4, 8, 12, 16, 20], "itemsize": 24})   # mx_limiter_tick
_proto("mx_graph_set_limiters", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
_proto("mx_graph_read_limiters", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t)
_proto("mx_graph_read_limited", C.c_int, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t))
_proto("mx_graph_read_limited_i16", C.c_int, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t))
_proto("mx_graph_limited_device_ptr", C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t))
_proto("mx_limiter_weights", C.c_int, C.c_uint32, C.c_void_p)
class TempoParams(C.Structure):
    """mx_tempo_params: frames per hop (64, 128, 256), the window in hops (64 .. 4096), the lags (16 .. 1024, <= window) and the emission period."""
    _fields_ = [("hop_frames", C.c_uint32), ("window_hops", C.c_uint32), ("max_lag", C.c_uint32), ("emit_ticks", C.c_uint32)]


_proto("mx_graph_set_tempo", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
_proto("mx_graph_read_tempo", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32))
_proto("mx_tempo_record_bytes", C.c_int, C.POINTER(TempoParams), C.POINTER(C.c_size_t))
_proto("mx_tempo_bpm", C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double))
class TonalityParams(C.Structure):
    """mx_tonality_params: decimation (4, 8), the hop in decimated frames (128, 256, 512), octaves (2 .. 6; 12 bins each), the lowest bin's
    frequency in millihertz and the emission period."""
    _fields_ = [("decim", C.c_uint32), ("hop_frames", C.c_uint32), ("octaves", C.c_uint32), ("f_lo_mhz", C.c_uint32), ("emit_ticks", C.c_uint32)]


_proto("mx_graph_set_tonality", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
_proto("mx_graph_read_tonality", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32))
_proto("mx_tonality_record_bytes", C.c_int, C.POINTER(TonalityParams), C.POINTER(C.c_size_t))
_proto("mx_tonality_tables", C.c_int, C.c_double, C.POINTER(TonalityParams), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t))
_proto("mx_tonality_chroma", C.c_int, C.c_void_p, C.c_size_t, C.c_double, C.POINTER(C.c_double))
_proto("mx_tonality_key", C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double))
class VideoScopeParams(C.Structure):
    """mx_video_scope_params: waveform columns (0, 64, 128, 256), vectorscope on / off, record every hop-th video tick."""
    _fields_ = [("wave_cols", C.c_uint32), ("vectorscope", C.c_uint32), ("hop", C.c_uint32)]


_proto("mx_graph_set_video_scopes", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
_proto("mx_graph_read_video_scopes", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32))
_proto("mx_video_scope_record_bytes", C.c_int, C.POINTER(VideoScopeParams), C.POINTER(C.c_size_t))
KEY_CHROMA, KEY_LUMA = 0, 1


class VideoKeyParams(C.Structure):
    """mx_video_key_params (24 bytes): the keyer's mode, key colour, ramp and spill distances in 1/16 of a code value."""
    _fields_ = [("mode", C.c_uint32), ("key_u", C.c_uint8), ("key_v", C.c_uint8), ("invert", C.c_uint8), ("_pad", C.c_uint8),
                ("near_q4", C.c_uint32), ("far_q4", C.c_uint32), ("spill_far_q4", C.c_uint32), ("spill_strength", C.c_uint32)]


_proto("mx_video_key", C.c_int, C.c_void_p, C.POINTER(VideoKeyParams), C.POINTER(C.c_void_p), C.c_void_p)
_proto("mx_graph_set_video_source_key", C.c_int, C.c_void_p, C.c_uint32, C.POINTER(VideoKeyParams))


GRADE_CURVE, GRADE_CHROMA, GRADE_LUT = 1, 2, 4


class VideoGradeParams(C.Structure):
    """mx_video_grade_params (284 bytes): the stages' flag bits, the luma curve, the Q12 chroma matrix (rows u, v) and offsets."""
    _fields_ = [("flags", C.c_uint32), ("curve_y", C.c_uint8 * 256), ("m_uu", C.c_int32), ("m_uv", C.c_int32), ("m_vu", C.c_int32), ("m_vv", C.c_int32),
                ("off_u", C.c_int32), ("off_v", C.c_int32)]


_proto("mx_video_lut_create", C.c_int, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p))
_proto("mx_video_lut_retain", C.c_int, C.c_void_p)
_proto("mx_video_lut_release", None, C.c_void_p)
_proto("mx_video_lut_identity", C.c_int, C.c_uint32, C.c_void_p)
_proto("mx_video_grade_procamp", C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(VideoGradeParams))
_proto("mx_video_grade", C.c_int, C.c_void_p, C.POINTER(VideoGradeParams), C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p)
_proto("mx_graph_set_video_source_grade", C.c_int, C.c_void_p, C.c_uint32, C.POINTER(VideoGradeParams), C.c_void_p)


MATTE_CLEAN, MATTE_CHOKE, MATTE_SOFTEN, MATTE_MASK = 1, 2, 4, 8
MATTE_MASK_RECT, MATTE_MASK_CIRCLE = 0, 1
WIPE_LEFT, WIPE_TOP, WIPE_BOX, WIPE_IRIS = 0, 1, 2, 3


class VideoMatteParams(C.Structure):
    """mx_video_matte_params (36 bytes): the stages' flag bits, the clean points, the choke and soften radii, the mask's shape, Q4 geometry and feather."""
    _fields_ = [("flags", C.c_uint32), ("clean_black", C.c_uint8), ("clean_white", C.c_uint8), ("choke", C.c_int8), ("soften", C.c_uint8),
                ("mask_shape", C.c_uint32), ("mask_invert", C.c_uint32), ("mask_x0", C.c_int32), ("mask_y0", C.c_int32), ("mask_x1", C.c_int32),
                ("mask_y1", C.c_int32), ("mask_feather_q4", C.c_uint32)]


_proto("mx_video_matte", C.c_int, C.c_void_p, C.POINTER(VideoMatteParams), C.POINTER(C.c_void_p), C.c_void_p)
_proto("mx_video_matte_check", C.c_int, C.POINTER(VideoMatteParams))
_proto("mx_video_matte_wipe", C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(VideoMatteParams))
_proto("mx_graph_set_video_source_matte", C.c_int, C.c_void_p, C.c_uint32, C.POINTER(VideoMatteParams))


class VideoPlaceParams(C.Structure):
    """mx_video_place_params (40 bytes): the canvas, the crop of the input (0 x 0: the whole frame) and the rectangle of the canvas it is stretched into."""
    _fields_ = [("canvas_w", C.c_uint32), ("canvas_h", C.c_uint32), ("crop_x", C.c_uint32), ("crop_y", C.c_uint32), ("crop_w", C.c_uint32), ("crop_h", C.c_uint32),
                ("dst_x", C.c_int32), ("dst_y", C.c_int32), ("dst_w", C.c_uint32), ("dst_h", C.c_uint32)]


# the placer's kernel (mx_video.hpp MX_PLACE_*): a workgroup writes a PLACE_TILE_W x PLACE_TILE_H tile of one canvas PLANE (chroma planes: half the luma numbers);
# axes of up to PLACE_TAP_BOUND taps (downscales up to 4:1) take the LDS-tiled form, more taps the gather form: tests put sizes and ratios around them
PLACE_TILE_W, PLACE_TILE_H, PLACE_TAP_BOUND = 64, 16, 18
_proto("mx_video_place", C.c_int, C.c_void_p, C.POINTER(VideoPlaceParams), C.POINTER(C.c_void_p), C.c_void_p)
_proto("mx_graph_set_video_source_place", C.c_int, C.c_void_p, C.c_uint32, C.POINTER(VideoPlaceParams))
MULTIVIEW_MAX = 16


class MultiviewView(C.Structure):
    """mx_multiview_view (24 bytes): a view's rectangle on the canvas (frame included), the tally frame's thickness and colour, and stretch (0) or keep-aspect (1)."""
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32), ("border", C.c_uint32),
                ("border_y", C.c_uint8), ("border_u", C.c_uint8), ("border_v", C.c_uint8), ("fit", C.c_uint8)]


class MultiviewParams(C.Structure):
    """mx_multiview_params (404 bytes): the canvas, its background colour, the views, and -- in a graph -- render every hop-th video tick."""
    _fields_ = [("canvas_w", C.c_uint32), ("canvas_h", C.c_uint32), ("bg_y", C.c_uint8), ("bg_u", C.c_uint8), ("bg_v", C.c_uint8), ("_pad", C.c_uint8),
                ("n_views", C.c_uint32), ("hop", C.c_uint32), ("view", MultiviewView * MULTIVIEW_MAX)]


class MultiviewStatus(C.Structure):
    """mx_multiview_status (16 bytes): recorded ticks of the last run, the tick rendered, which ports held a frame, which views were shown."""
    _fields_ = [("recorded", C.c_uint32), ("tick_in_run", C.c_uint32), ("present_mask", C.c_uint32), ("shown_mask", C.c_uint32)]


# the multiviewer's kernel (mx_video.hpp MX_MULTIVIEW_*): a workgroup writes a MULTIVIEW_TILE_W x MULTIVIEW_TILE_H tile of one canvas PLANE (chroma planes: half the
# luma numbers); axes of up to MULTIVIEW_TAP_BOUND taps (downscales up to 4.5:1) take the LDS-tiled form, more taps the gather form: tests put sizes and ratios around them
MULTIVIEW_TILE_W, MULTIVIEW_TILE_H, MULTIVIEW_TAP_BOUND = 64, 16, 20
_proto("mx_video_multiview", C.c_int, C.POINTER(C.c_void_p), C.POINTER(MultiviewParams), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_void_p)
_proto("mx_graph_set_multiview", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(MultiviewParams))
_proto("mx_graph_multiview_output", C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(MultiviewStatus))
_proto("mx_graph_profile_run", C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float))
_proto("mx_graph_profile_enable", C.c_int, C.c_void_p, C.c_int)
_proto("mx_graph_profile_collect", C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint32))


class PerformanceInfo(C.Structure):
    """mx_performance_info (PerformanceInfo, protocol/src/lib.rs:32-59)."""
    _fields_ = [("realtime", C.c_int32), ("lag", C.c_int32), ("tick_rate", C.c_uint32), ("n_modules", C.c_uint32),
                ("tick_budget_us", C.c_uint64), ("engine_us", C.c_uint64)]


_proto("mx_graph_performance_info", C.c_int, C.c_void_p, C.POINTER(PerformanceInfo), C.POINTER(C.c_uint64), C.c_size_t)
_proto("mx_graph_adopt_state", C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_size_t)
_proto("mx_pcm_ring_create", C.c_int, C.POINTER(C.c_void_p))
_proto("mx_pcm_ring_destroy", None, C.c_void_p)
_proto("mx_pcm_ring_push_i16", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
_proto("mx_pcm_ring_queued", C.c_int, C.c_void_p, C.POINTER(C.c_size_t))
_proto("mx_pcm_ring_feed", C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_size_t))
# the deck (mixlab_amd/deck.py): a track in device memory played at variable speed into a SOURCE_STEREO node
DECK_PLAY, DECK_LOOP = 1, 2
DECK_TICK_PLAY, DECK_TICK_LOOPING, DECK_TICK_BEFORE, DECK_TICK_PAST = 1, 2, 4, 8
DECK_TAPS, DECK_PHASES, DECK_BANKS = 32, 256, 4
DECK_CHUNK = 256          # MX_DECK_CHUNK: output frames one workgroup of the feed kernel writes
DECK_MAX_SPT = 1 << 20    # MX_DECK_MAX_SPT
class DeckParams(C.Structure):
    _fields_ = [("step_q32", C.c_int64), ("slew_q32", C.c_int64), ("loop_in", C.c_int64), ("loop_out", C.c_int64), ("flags", C.c_uint32), ("_pad", C.c_uint32)]
class DeckHead(C.Structure):
    _fields_ = [("pos_q32", C.c_int64), ("step_q32", C.c_int64), ("params", DeckParams), ("last_loop_in", C.c_int64), ("last_loop_out", C.c_int64),
                ("last_looping", C.c_uint32), ("_pad", C.c_uint32)]
class DeckTick(C.Structure):
    _fields_ = [("pos_q32", C.c_int64), ("step_q32", C.c_int64), ("dstep_q32", C.c_int64), ("loop_in", C.c_int64), ("loop_len", C.c_int64),
                ("flags", C.c_uint32), ("bank", C.c_uint32)]
_proto("mx_deck_create", C.c_int, C.c_uint64, C.c_int, C.POINTER(C.c_void_p))
_proto("mx_deck_destroy", None, C.c_void_p)
_proto("mx_deck_load_i16", C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64)
_proto("mx_deck_set", C.c_int, C.c_void_p, C.POINTER(DeckParams))
_proto("mx_deck_seek", C.c_int, C.c_void_p, C.c_int64)
_proto("mx_deck_schedule", C.c_int, C.c_void_p, C.c_uint32, C.POINTER(DeckParams), C.POINTER(C.c_int64))
_proto("mx_deck_check", C.c_int, C.POINTER(DeckParams), C.c_uint64)
_proto("mx_deck_plan", C.c_int, C.POINTER(DeckHead), C.POINTER(DeckParams), C.POINTER(C.c_int64), C.c_uint32, C.c_uint64, C.POINTER(DeckTick), C.POINTER(DeckHead))
_proto("mx_deck_feed", C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_size_t, C.c_void_p, C.c_uint32)
_proto("mx_deck_read_ticks", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DeckTick))
_proto("mx_deck_state", C.c_int, C.c_void_p, C.POINTER(DeckHead))
_proto("mx_deck_step", C.c_int, C.c_uint32, C.c_uint32, C.c_double, C.POINTER(C.c_int64))
_proto("mx_deck_tables", C.c_int, C.c_uint32, C.c_void_p)
_proto("mx_deck_debug_last_feed", C.c_int, C.POINTER(C.c_uint32))
# ... key-locked (the header's KEY-LOCK): tempo without pitch change by overlap-add of searched grains
DECK_GRAIN_FIRST = 1
class DeckKeylock(C.Structure):
    _fields_ = [("pitch_q32", C.c_int64), ("hop", C.c_uint32), ("overlap", C.c_uint32), ("radius", C.c_uint32), ("_pad", C.c_uint32)]
class DeckGrain(C.Structure):
    _fields_ = [("a_q32", C.c_int64), ("g_q32", C.c_int64), ("tick", C.c_uint32), ("frame", C.c_uint32), ("delta", C.c_int32), ("dist", C.c_uint32),
                ("flags", C.c_uint32), ("_pad", C.c_uint32)]
_proto("mx_deck_set_keylock", C.c_int, C.c_void_p, C.POINTER(DeckKeylock))
_proto("mx_deck_keylock_check", C.c_int, C.POINTER(DeckKeylock))
_proto("mx_deck_keylock_search", C.c_int, C.c_void_p, C.c_uint64, C.c_int64, C.c_int64, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_uint32))
_proto("mx_deck_grain_count", C.c_int, C.c_void_p, C.POINTER(C.c_uint32))
_proto("mx_deck_read_grains", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DeckGrain))
_proto("mx_deck_debug_last_keylock", C.c_int, C.POINTER(C.c_uint32))
# ... analysed (the header's ANALYSIS): band waveform columns, onset autocorrelation and beat grid of the whole track
DECK_ANALYSIS_MAX_TAPS = 127
class DeckAnalysis(C.Structure):
    _fields_ = [("column", C.c_uint32), ("taps", C.c_uint32), ("max_lag", C.c_uint32), ("_pad", C.c_uint32),
                ("lo", C.c_int16 * DECK_ANALYSIS_MAX_TAPS), ("hi", C.c_int16 * DECK_ANALYSIS_MAX_TAPS)]
class DeckColumn(C.Structure):
    _fields_ = [("smin", C.c_int32), ("smax", C.c_int32), ("peak", C.c_uint32 * 3), ("onset", C.c_uint32), ("energy", C.c_uint64 * 3), ("e", C.c_uint64)]
class DeckGrid(C.Structure):
    _fields_ = [("bpm", C.c_double), ("period_columns", C.c_double), ("confidence", C.c_double), ("first_beat_frame", C.c_uint64),
                ("lag", C.c_uint32), ("phase_column", C.c_uint32)]
_proto("mx_deck_analysis_check", C.c_int, C.POINTER(DeckAnalysis))
_proto("mx_deck_analysis_bands", C.c_int, C.c_double, C.c_double, C.c_double, C.c_uint32, C.POINTER(DeckAnalysis))
_proto("mx_deck_analyse", C.c_int, C.c_void_p, C.POINTER(DeckAnalysis))
_proto("mx_deck_column_count", C.c_int, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64))
_proto("mx_deck_read_columns", C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p)
_proto("mx_deck_read_autocorr", C.c_int, C.c_void_p, C.c_void_p, C.c_uint32)
_proto("mx_deck_columns_host", C.c_int, C.c_void_p, C.c_uint64, C.POINTER(DeckAnalysis), C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p)
_proto("mx_deck_beatgrid", C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_double, C.POINTER(DeckGrid))
_proto("mx_deck_debug_last_analysis", C.c_int, C.POINTER(C.c_uint32))
# ... its key and loudness (the header's KEY AND LOUDNESS): the tonality and loudness taps' rules over the whole track
class DeckTonality(C.Structure):
    _fields_ = [("rate", C.c_double), ("decim", C.c_uint32), ("hop_frames", C.c_uint32), ("octaves", C.c_uint32), ("f_lo_mhz", C.c_uint32),
                ("segment_hops", C.c_uint32), ("_pad", C.c_uint32)]
class DeckLoudness(C.Structure):
    _fields_ = [("rate", C.c_double), ("block_frames", C.c_uint32), ("momentary_blocks", C.c_uint32), ("short_blocks", C.c_uint32), ("_pad", C.c_uint32)]
_proto("mx_deck_tonality_check", C.c_int, C.POINTER(DeckTonality))
_proto("mx_deck_tonality_count", C.c_int, C.c_uint64, C.POINTER(DeckTonality), C.POINTER(C.c_uint64))
_proto("mx_deck_analyse_tonality", C.c_int, C.c_void_p, C.POINTER(DeckTonality))
_proto("mx_deck_read_tonality", C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_size_t)
_proto("mx_deck_tonality_host", C.c_int, C.c_void_p, C.c_uint64, C.POINTER(DeckTonality), C.c_uint64, C.c_uint64, C.c_void_p)
_proto("mx_deck_debug_last_tonality", C.c_int, C.POINTER(C.c_uint32))
_proto("mx_deck_loudness_check", C.c_int, C.POINTER(DeckLoudness))
_proto("mx_deck_loudness_count", C.c_int, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64))
_proto("mx_deck_analyse_loudness", C.c_int, C.c_void_p, C.POINTER(DeckLoudness))
_proto("mx_deck_read_loudness", C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p)
_proto("mx_deck_loudness_host", C.c_int, C.c_void_p, C.c_uint64, C.POINTER(DeckLoudness), C.c_void_p, C.c_uint64)
_proto("mx_deck_debug_last_loudness", C.c_int, C.POINTER(C.c_uint32))
_proto("mx_deck_loudness_gain", C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
       C.POINTER(C.c_double))
_proto("mx_tonality_camelot", C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))
# ... its fine beat grid and sync (the header's FINE GRID): a comb search over candidate periods and phases, and the arithmetic that aligns two decks
DECK_FINEGRID_LANES = 256          # MX_DECK_FINEGRID_LANES: phases one pass of a comb workgroup covers
DECK_FINEGRID_MAX_PERIODS = 8192   # MX_DECK_FINEGRID_MAX_PERIODS
class DeckFinegrid(C.Structure):
    _fields_ = [("hop", C.c_uint32), ("n_periods", C.c_uint32), ("period0_q16", C.c_uint64), ("dperiod_q16", C.c_uint32), ("first_hop", C.c_uint32),
                ("max_beats", C.c_uint32), ("_pad", C.c_uint32)]
class DeckComb(C.Structure):
    _fields_ = [("score", C.c_uint64), ("phase", C.c_uint32), ("beats", C.c_uint32)]
class DeckBeats(C.Structure):
    _fields_ = [("first_q32", C.c_int64), ("period_q32", C.c_int64)]
class DeckFinePick(C.Structure):
    _fields_ = [("grid", DeckBeats), ("score", C.c_uint64), ("bpm", C.c_double), ("index", C.c_uint32), ("n_beats", C.c_uint32)]
class DeckSyncResult(C.Structure):
    _fields_ = [("step_q32", C.c_int64), ("seek_q32", C.c_int64), ("delta_q32", C.c_int64)]
DECK_COMB_DTYPE = np.dtype([("score", "<u8"), ("phase", "<u4"), ("beats", "<u4")])   # mx_deck_comb as a numpy record: 16 bytes
_proto("mx_deck_finegrid_check", C.c_int, C.POINTER(DeckFinegrid), C.c_uint64)
_proto("mx_deck_finegrid_count", C.c_int, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64))
_proto("mx_deck_finegrid_span", C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(DeckFinegrid), C.POINTER(C.c_uint32))
_proto("mx_deck_finegrid_period", C.c_int, C.c_double, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64))
_proto("mx_deck_analyse_finegrid", C.c_int, C.c_void_p, C.POINTER(DeckFinegrid))
_proto("mx_deck_read_finegrid", C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p)
_proto("mx_deck_read_fine_onsets", C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p)
_proto("mx_deck_finegrid_host", C.c_int, C.c_void_p, C.c_uint64, C.POINTER(DeckFinegrid), C.c_void_p, C.c_void_p)
_proto("mx_deck_finegrid_pick", C.c_int, C.c_void_p, C.POINTER(DeckFinegrid), C.c_double, C.POINTER(DeckFinePick))
_proto("mx_deck_sync", C.c_int, C.POINTER(DeckBeats), C.c_int64, C.c_int64, C.POINTER(DeckBeats), C.c_int64, C.POINTER(DeckSyncResult))
_proto("mx_deck_debug_last_finegrid", C.c_int, C.POINTER(C.c_uint32))
# ... its beat echo (the header's ECHO): a feedback delay per deck behind the feed, scheduled per tick
DECK_ECHO_PINGPONG = 1
DECK_ECHO_MIN_DELAY, DECK_ECHO_MAX_DELAY = 256, 262144
class DeckEcho(C.Structure):
    _fields_ = [("delay", C.c_uint32), ("flags", C.c_uint32), ("send", C.c_float), ("feedback", C.c_float), ("wet", C.c_float), ("damp", C.c_float)]
_proto("mx_deck_set_echo", C.c_int, C.c_void_p, C.POINTER(DeckEcho))
_proto("mx_deck_schedule_echo", C.c_int, C.c_void_p, C.c_uint32, C.POINTER(DeckEcho))
_proto("mx_deck_echo_check", C.c_int, C.POINTER(DeckEcho))
_proto("mx_deck_echo_delay", C.c_int, C.POINTER(DeckBeats), C.c_int64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32))
_proto("mx_deck_echo_state", C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(DeckEcho))
_proto("mx_deck_echo_plan", C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32))
_proto("mx_deck_debug_last_echo", C.c_int, C.POINTER(C.c_uint32))
# ... its sweep filter (the header's FILTER): a resonant state-variable filter per deck between the feed and the echo, scheduled per tick
DECK_FILTER_LP, DECK_FILTER_HP, DECK_FILTER_BP, DECK_FILTER_NOTCH = 0, 1, 2, 3
DECK_FILTER_MIN_G, DECK_FILTER_MAX_G = 2.0 ** -12, 16.0
DECK_FILTER_MIN_K, DECK_FILTER_MAX_K = 0.05000000074505806, 2.0   # (0.05 as an f32)
class DeckFilter(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("flags", C.c_uint32), ("g", C.c_float), ("k", C.c_float), ("wet", C.c_float), ("_pad", C.c_uint32)]
class DeckFilterCarry(C.Structure):
    _fields_ = [("s", C.c_double * 4), ("last", DeckFilter), ("on", C.c_uint32), ("_pad", C.c_uint32)]
_proto("mx_deck_set_filter", C.c_int, C.c_void_p, C.POINTER(DeckFilter))
_proto("mx_deck_schedule_filter", C.c_int, C.c_void_p, C.c_uint32, C.POINTER(DeckFilter))
_proto("mx_deck_filter_check", C.c_int, C.POINTER(DeckFilter))
_proto("mx_deck_filter_state", C.c_int, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(DeckFilter))
_proto("mx_deck_read_filter_state", C.c_int, C.c_void_p, C.POINTER(C.c_double))
_proto("mx_deck_filter_design", C.c_int, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(DeckFilter))
_proto("mx_deck_filter_knob", C.c_int, C.c_double, C.c_double, C.c_double, C.POINTER(DeckFilter), C.POINTER(C.c_uint32))
_proto("mx_deck_filter_host", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(DeckFilterCarry))
_proto("mx_deck_debug_last_filter", C.c_int, C.POINTER(C.c_uint32))
# ... its reverb (the header's REVERB): a feedback delay network per deck behind the echo, scheduled per tick
DECK_REVERB_MIN_DELAY, DECK_REVERB_MAX_DELAY = 128, 12000
DECK_REVERB_MIN_DIFF, DECK_REVERB_MAX_DIFF = 64, 2000
DECK_REVERB_TANK_RING, DECK_REVERB_DIFF_RING = 16384, 4096
DECK_REVERB_LINE_FLOATS = 8 * 16384 + 4 * 4096
class DeckReverb(C.Structure):
    _fields_ = [("delay", C.c_uint32 * 8), ("diff", C.c_uint32 * 4), ("gain", C.c_float * 8), ("send", C.c_float), ("dry", C.c_float), ("wet", C.c_float),
                ("damp", C.c_float), ("diffusion", C.c_float), ("flags", C.c_uint32)]
class DeckReverbCarry(C.Structure):
    _fields_ = [("t", C.c_uint64), ("last", DeckReverb), ("on", C.c_uint32), ("_pad", C.c_uint32)]
_proto("mx_deck_set_reverb", C.c_int, C.c_void_p, C.POINTER(DeckReverb))
_proto("mx_deck_schedule_reverb", C.c_int, C.c_void_p, C.c_uint32, C.POINTER(DeckReverb))
_proto("mx_deck_reverb_check", C.c_int, C.POINTER(DeckReverb))
_proto("mx_deck_reverb_state", C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(DeckReverb))
_proto("mx_deck_read_reverb_lines", C.c_int, C.c_void_p, C.c_void_p)
_proto("mx_deck_reverb_plan", C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32))
_proto("mx_deck_reverb_host", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(DeckReverbCarry))
_proto("mx_deck_reverb_design", C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(DeckReverb))
_proto("mx_deck_debug_last_reverb", C.c_int, C.POINTER(C.c_uint32))
# ... its bars and phrases (the header's BARS): beat vectors, checkerboard novelty at two widths, and the folds the downbeat and the phrase line are picked from
DECK_BARS_MAX_BEATS = 16384   # MX_DECK_BARS_MAX_BEATS
DECK_BARS_MAX_FOLDS = 136     # MX_DECK_BARS_MAX_FOLDS
DECK_BARS_BLOCK = 4           # MX_DECK_BARS_BLOCK: beats one novelty workgroup takes
class DeckBars(C.Structure):
    _fields_ = [("grid", DeckBeats), ("lead", C.c_uint32), ("taps", C.c_uint32), ("beats_per_bar", C.c_uint32), ("bars_per_phrase", C.c_uint32), ("w_bar", C.c_uint32),
                ("w_phrase", C.c_uint32), ("max_beats", C.c_uint32), ("lo", C.c_int16 * DECK_ANALYSIS_MAX_TAPS), ("hi", C.c_int16 * DECK_ANALYSIS_MAX_TAPS)]
class DeckBeat(C.Structure):
    _fields_ = [("v", C.c_uint32 * 6), ("first_frame", C.c_uint32), ("frames", C.c_uint32), ("n_bar", C.c_int64), ("n_phrase", C.c_int64)]
class DeckBarPick(C.Structure):
    _fields_ = [("bars", DeckBeats), ("phrases", DeckBeats), ("bar_phase", C.c_uint32), ("phrase_phase", C.c_uint32), ("bar_best", C.c_uint64), ("bar_sum", C.c_uint64),
                ("phrase_best", C.c_uint64), ("phrase_sum", C.c_uint64)]
DECK_BEAT_DTYPE = np.dtype([("v", "<u4", (6,)), ("first_frame", "<u4"), ("frames", "<u4"), ("n_bar", "<i8"), ("n_phrase", "<i8")])   # mx_deck_beat as a numpy record: 48 bytes
_proto("mx_deck_bars_check", C.c_int, C.POINTER(DeckBars), C.c_uint64)
_proto("mx_deck_bars_count", C.c_int, C.POINTER(DeckBars), C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_int64))
_proto("mx_deck_bars_tables", C.c_int, C.POINTER(DeckAnalysis), C.POINTER(DeckBars))
_proto("mx_deck_analyse_bars", C.c_int, C.c_void_p, C.POINTER(DeckBars))
_proto("mx_deck_read_bars", C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p)
_proto("mx_deck_read_bar_folds", C.c_int, C.c_void_p, C.c_void_p, C.c_uint32)
_proto("mx_deck_bars_host", C.c_int, C.c_void_p, C.c_uint64, C.POINTER(DeckBars), C.c_void_p, C.c_void_p)
_proto("mx_deck_bars_pick", C.c_int, C.c_void_p, C.POINTER(DeckBars), C.POINTER(DeckBarPick))
_proto("mx_deck_grid_next", C.c_int, C.POINTER(DeckBeats), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64))
_proto("mx_deck_debug_last_bars", C.c_int, C.POINTER(C.c_uint32))
# ... its tempo map (the header's TEMPO MAP): the comb search per window of the track, the path through the windows, segments, look-up and warp
DECK_TEMPOMAP_MAX_WINDOW = 16384       # MX_DECK_TEMPOMAP_MAX_WINDOW
DECK_TEMPOMAP_MAX_PERIODS = 1024       # MX_DECK_TEMPOMAP_MAX_PERIODS
DECK_TEMPOMAP_MAX_RECORDS = 1 << 20    # MX_DECK_TEMPOMAP_MAX_RECORDS
DECK_TEMPOMAP_GROUP = 8                # MX_DECK_TEMPOMAP_GROUP: candidates one comb workgroup walks
DECK_TEMPOMAP_STAGED_MAX = 10112     # MX_DECK_TEMPOMAP_STAGED_MAX: the longest window a comb workgroup stages in LDS
DECK_TEMPO_EMPTY = 1                   # MX_DECK_TEMPO_EMPTY
class DeckTempomap(C.Structure):
    _fields_ = [("hop", C.c_uint32), ("n_periods", C.c_uint32), ("period0_q16", C.c_uint64), ("dperiod_q16", C.c_uint32), ("window_hops", C.c_uint32),
                ("stride_hops", C.c_uint32), ("_pad", C.c_uint32)]
class DeckTempoSegment(C.Structure):
    _fields_ = [("start_q32", C.c_int64), ("grid", DeckBeats), ("score", C.c_uint64), ("window", C.c_uint32), ("flags", C.c_uint32)]
DECK_TEMPO_SEGMENT_DTYPE = np.dtype([("start_q32", "<i8"), ("first_q32", "<i8"), ("period_q32", "<i8"), ("score", "<u8"), ("window", "<u4"), ("flags", "<u4")])   # 40 bytes, the grid flat
_proto("mx_deck_tempomap_check", C.c_int, C.POINTER(DeckTempomap), C.c_uint64)
_proto("mx_deck_tempomap_count", C.c_int, C.POINTER(DeckTempomap), C.c_uint64, C.POINTER(C.c_uint32))
_proto("mx_deck_tempomap_span", C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(DeckTempomap), C.POINTER(C.c_uint32))
_proto("mx_deck_tempomap_host", C.c_int, C.c_void_p, C.c_uint64, C.POINTER(DeckTempomap), C.c_void_p, C.c_void_p)
_proto("mx_deck_tempomap_path", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p)
_proto("mx_deck_tempomap_segments", C.c_int, C.c_void_p, C.POINTER(DeckTempomap), C.c_uint64, C.c_void_p, C.c_void_p)
_proto("mx_deck_tempomap_at", C.c_int, C.c_void_p, C.c_uint32, C.c_int64, C.POINTER(DeckBeats), C.POINTER(C.c_uint32))
_proto("mx_deck_tempomap_step", C.c_int, C.POINTER(DeckBeats), C.c_int64, C.POINTER(C.c_int64))
_proto("mx_deck_analyse_tempomap", C.c_int, C.c_void_p, C.POINTER(DeckTempomap))
_proto("mx_deck_read_tempomap", C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p)
_proto("mx_deck_read_tempomap_onsets", C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p)
_proto("mx_deck_debug_last_tempomap", C.c_int, C.POINTER(C.c_uint32))
# ... its waveform picture (the header's WAVEFORM): the columns rendered to a yuv420p frame on the device, with beat lines, markers and ranges
WAVE_BANDS, WAVE_ENVELOPE = 0, 1       # MX_WAVE_BANDS, MX_WAVE_ENVELOPE
WAVE_MAX_GRIDS, WAVE_MAX_MARKERS, WAVE_MAX_RANGES = 16, 32, 8
WAVE_STRIP = 64                        # MX_WAVE_STRIP: pixel columns one workgroup renders
class WaveColour(C.Structure):
    _fields_ = [("y", C.c_uint8), ("u", C.c_uint8), ("v", C.c_uint8), ("_pad", C.c_uint8)]
class WaveGrid(C.Structure):
    _fields_ = [("grid", DeckBeats), ("from_q32", C.c_int64), ("to_q32", C.c_int64), ("colour", WaveColour), ("inset", C.c_uint32)]
class WaveMarker(C.Structure):
    _fields_ = [("frame", C.c_int64), ("width", C.c_uint32), ("colour", WaveColour)]
class WaveRange(C.Structure):
    _fields_ = [("from_frame", C.c_int64), ("to_frame", C.c_int64), ("colour", WaveColour), ("_pad", C.c_uint32)]
class DeckWaveform(C.Structure):
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("first_frame", C.c_int64), ("frames_per_px", C.c_uint32), ("style", C.c_uint32), ("gain_q16", C.c_uint32 * 3),
                ("bg", WaveColour), ("line", WaveColour), ("band", WaveColour * 3), ("n_grids", C.c_uint32), ("n_markers", C.c_uint32), ("n_ranges", C.c_uint32),
                ("_pad", C.c_uint32), ("grid", WaveGrid * WAVE_MAX_GRIDS), ("marker", WaveMarker * WAVE_MAX_MARKERS), ("range", WaveRange * WAVE_MAX_RANGES)]
_proto("mx_deck_waveform_check", C.c_int, C.POINTER(DeckWaveform))
_proto("mx_deck_waveform_view", C.c_int, C.c_int64, C.c_uint32, C.c_uint32, C.POINTER(C.c_int64))
_proto("mx_deck_render_waveform", C.c_int, C.c_void_p, C.POINTER(DeckWaveform), C.POINTER(C.c_void_p), C.c_void_p)
_proto("mx_deck_waveform_host", C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.POINTER(DeckWaveform), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32)
_proto("mx_deck_debug_last_waveform", C.c_int, C.POINTER(C.c_uint32))
_proto("mx_module_create", C.c_int, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p))
_proto("mx_module_create_ex", C.c_int, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(GraphOpts), C.POINTER(C.c_void_p))
_proto("mx_module_update", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
_proto("mx_module_run_tick", C.c_int, C.c_void_p, C.c_uint64, C.POINTER(Input), C.c_size_t, C.POINTER(Output), C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t))
_proto("mx_module_destroy", None, C.c_void_p)


class MxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"mixlab_gpu error {code}: {msg}")
        self.code = code


def spectrum_tables(n_fft: int):
    """(window[n_fft], twiddle_re[n_fft // 2], twiddle_im[n_fft // 2]) float32: the tables the spectrum kernels use (host only, no device)"""
    if n_fft not in (256, 512, 1024, 2048, 4096):   # before any buffer is sized from it
        raise MxError(MX_ERR_INVALID, "n_fft must be 256, 512, 1024, 2048 or 4096")
    w, re, im = np.zeros(n_fft, np.float32), np.zeros(n_fft // 2, np.float32), np.zeros(n_fft // 2, np.float32)
    check(lib.mx_spectrum_tables(n_fft, w.ctypes.data_as(C.c_void_p), re.ctypes.data_as(C.c_void_p), im.ctypes.data_as(C.c_void_p)))
    return w, re, im


def loudness_tables(rate: float, frames_per_tick: int):
    """(biquads float64[10]: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2; carry float64[4, 4]; interp float32[3, 12]): the tables the
    loudness kernels use for a port of that rate and tick length (host only, no device)"""
    bq, carry, interp = np.zeros(10), np.zeros((4, 4)), np.zeros((3, 12), np.float32)
    check(lib.mx_loudness_tables(float(rate), int(frames_per_tick), bq.ctypes.data_as(C.c_void_p), carry.ctypes.data_as(C.c_void_p),
                                 interp.ctypes.data_as(C.c_void_p)))
    return bq, carry, interp


def lufs(sq, frames):
    """loudness in LUFS of a K-weighted sum of squares over `frames` frames per channel (a record's momentary_sq over momentary_ticks x
    frames, short_sq over short_ticks x frames, ksq[0] + ksq[1] over frames): -0.691 + 10 log10(sq / frames); silence reads -inf"""
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(np.asarray(sq, np.float64) / np.asarray(frames, np.float64))


def loudness_gate(block_sq, block_frames):
    """(integrated loudness in LUFS, blocks kept) of BS.1770-4's two-stage gating over measurement blocks (mx_loudness_gate, host only):
    block_sq[i] is a momentary_sq, block_frames[i] (or one number for all) its frames; feed every 6th tick at 60 ticks/s"""
    sq = np.ascontiguousarray(block_sq, np.float64)
    fr = np.ascontiguousarray(np.broadcast_to(np.asarray(block_frames, np.uint32), sq.shape))
    out, kept = C.c_double(), C.c_size_t()
    check(lib.mx_loudness_gate(sq.ctypes.data_as(C.c_void_p), fr.ctypes.data_as(C.c_void_p), sq.size, C.byref(out), C.byref(kept)))
    return out.value, kept.value


def limiter_weights(lookahead: int) -> np.ndarray:
    """float32[lookahead + 1]: the smoothing weights the limiter kernel uses (mx_limiter_weights, host only, no device)"""
    if not 0 <= int(lookahead) <= LIMITER_MAX_LOOKAHEAD:   # before any buffer is sized from it
        raise MxError(MX_ERR_INVALID, "lookahead must be 0 .. 512")
    w = np.zeros(int(lookahead) + 1, np.float32)
    check(lib.mx_limiter_weights(int(lookahead), w.ctypes.data_as(C.c_void_p)))
    return w


def stereo_gonio_record_bytes(grid: int) -> int:
    """bytes of one goniometer record: 32 + 4 * grid * grid (host only, no device)"""
    n = C.c_size_t()
    check(lib.mx_stereo_gonio_record_bytes(C.byref(StereoParams(1, int(grid), 0, 1)), C.byref(n)))
    return n.value


def stereo_correlation(ll: float, rr: float, lr: float) -> float:
    """phase correlation lr / sqrt(ll * rr) of a record's sums or window sums, clamped to [-1, 1]; 0.0 when ll * rr is not a positive finite
    number (mx_stereo_correlation, host only)"""
    r = C.c_double()
    check(lib.mx_stereo_correlation(float(ll), float(rr), float(lr), C.byref(r)))
    return r.value


def parse_goniometer_records(raw: np.ndarray, grid: int) -> list:
    """raw bytes of back-to-back goniometer records -> one dict per record: the header fields as ints and gon [grid, grid] uint32, indexed
    [cell(L + R), cell(L - R)]"""
    r = np.ascontiguousarray(raw).view(np.uint32).reshape(-1, 8 + grid * grid)
    out = []
    for w in r:
        d = dict(zip(("tick_in_run", "ticks", "frames", "skipped", "grid", "zoom_log2"), (int(x) for x in w[:6])))
        d["reserved"] = (int(w[6]), int(w[7]))
        d["gon"] = w[8:].reshape(grid, grid)
        out.append(d)
    return out


def tempo_record_bytes(hop_frames: int = 128, window_hops: int = 2048, max_lag: int = 512, emit_ticks: int = 6) -> int:
    """bytes of one tempo record: 32 + 8 * max_lag (mx_tempo_record_bytes, host only, no device)"""
    n = C.c_size_t()
    check(lib.mx_tempo_record_bytes(C.byref(TempoParams(int(hop_frames), int(window_hops), int(max_lag), int(emit_ticks))), C.byref(n)))
    return n.value


def parse_tempo_records(raw: np.ndarray, max_lag: int) -> list:
    """raw bytes of back-to-back tempo records -> one dict per record: the header fields as ints, acf uint64[max_lag] (R[l]) and raw, the
    record's own bytes (what tempo_bpm takes)"""
    r = np.ascontiguousarray(raw).view(np.uint8).reshape(-1, 32 + 8 * max_lag)
    out = []
    for b in r:
        w = b[:32].view(np.uint32)
        d = dict(zip(("tick_in_run", "hops_complete", "nonfinite", "hop_frames", "window_hops", "max_lag"), (int(x) for x in w[:6])))
        d["reserved"] = (int(w[6]), int(w[7]))
        d["acf"] = b[32:].view(np.uint64)
        d["raw"] = b.tobytes()
        out.append(d)
    return out


def tempo_bpm(record, rate: float, bpm_lo: float, bpm_hi: float):
    """(bpm, confidence) of one tempo record (its bytes, or a parse_tempo_records dict) for a port of `rate` frames per second, searched
    between bpm_lo and bpm_hi: the first maximum of the autocorrelation over the lags of that range, refined by a parabola; confidence is
    R[lag] / R[0]; silence reads (0.0, 0.0) (mx_tempo_bpm, host only)"""
    raw = record["raw"] if isinstance(record, dict) else bytes(record)
    buf = (C.c_char * len(raw)).from_buffer_copy(raw)
    b, c = C.c_double(), C.c_double()
    if len(raw) < 32 or len(raw) < 32 + 8 * int(np.frombuffer(raw, np.uint32, 8)[5]):   # before the library reads max_lag values from it
        raise MxError(MX_ERR_INVALID, "a tempo record is 32 + 8 * max_lag bytes")
    check(lib.mx_tempo_bpm(buf, float(rate), float(bpm_lo), float(bpm_hi), C.byref(b), C.byref(c)))
    return b.value, c.value


def tonality_record_bytes(decim: int = 8, hop_frames: int = 512, octaves: int = 5, f_lo_mhz: int = 65406, emit_ticks: int = 30) -> int:
    """bytes of one tonality record: 32 + 8 * 12 * octaves (mx_tonality_record_bytes, host only, no device)"""
    n = C.c_size_t()
    check(lib.mx_tonality_record_bytes(C.byref(TonalityParams(int(decim), int(hop_frames), int(octaves), int(f_lo_mhz), int(emit_ticks))), C.byref(n)))
    return n.value


def tonality_tables(rate: float, decim: int = 8, hop_frames: int = 512, octaves: int = 5, f_lo_mhz: int = 65406):
    """(fir int16[8 * decim], len uint32[12 * octaves], kern int16[sum(len)][2]) -- the decimator's taps, the kernels' lengths N_b and their
    {re, im} coefficients, bin after bin -- as the device uses them for a port of `rate` frames per second (mx_tonality_tables, host only)"""
    par = TonalityParams(int(decim), int(hop_frames), int(octaves), int(f_lo_mhz), 1)
    fir, ln, pairs = np.zeros(8 * max(0, int(decim)), np.int16), np.zeros(12 * max(0, int(octaves)), np.uint32), C.c_size_t()
    check(lib.mx_tonality_tables(float(rate), C.byref(par), fir.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p), None, C.byref(pairs)))
    kern = np.zeros((pairs.value, 2), np.int16)
    check(lib.mx_tonality_tables(float(rate), C.byref(par), fir.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p), kern.ctypes.data_as(C.c_void_p), C.byref(pairs)))
    return fir, ln, kern


def parse_tonality_records(raw: np.ndarray, octaves: int) -> list:
    """raw bytes of back-to-back tonality records -> one dict per record: the header fields as ints, cq uint64[12 * octaves] (C[b]) and raw,
    the record's own bytes (what tonality_chroma takes)"""
    r = np.ascontiguousarray(raw).view(np.uint8).reshape(-1, 32 + 96 * octaves)
    out = []
    for b in r:
        w = b[:32].view(np.uint32)
        d = dict(zip(("tick_in_run", "hops", "nonfinite", "decim", "hop_frames", "octaves", "f_lo_mhz", "reserved"), (int(x) for x in w)))
        d["cq"] = b[32:].view(np.uint64)
        d["raw"] = b.tobytes()
        out.append(d)
    return out


def tonality_chroma(records, rate: float) -> np.ndarray:
    """the pitch-class profile float64[12] (C = 0, sum 1 or all zero) of one tap's records -- bytes, or parse_tonality_records dicts --
    summed, for a port of `rate` frames per second (mx_tonality_chroma, host only)"""
    raw = b"".join(r["raw"] if isinstance(r, dict) else bytes(r) for r in records)
    if len(raw) < 32:
        raise MxError(MX_ERR_INVALID, "a tonality record is 32 + 96 * octaves bytes")
    rb = 32 + 96 * int(np.frombuffer(raw, np.uint32, 8)[5])   # before the library reads that many bytes per record
    if len(raw) % rb:
        raise MxError(MX_ERR_INVALID, "a tonality record is 32 + 96 * octaves bytes")
    buf = (C.c_char * len(raw)).from_buffer_copy(raw)
    out = (C.c_double * 12)()
    check(lib.mx_tonality_chroma(buf, len(raw) // rb, float(rate), out))
    return np.array(out[:], np.float64)


def tonality_key(chroma):
    """(key, confidence) of a pitch-class profile: key 0 .. 11 major on that tonic (C = 0), 12 .. 23 minor, -1 for a profile without
    variance; confidence the best Krumhansl-Kessler correlation minus the second best (mx_tonality_key, host only)"""
    c = (C.c_double * 12)(*[float(x) for x in chroma])
    k, conf = C.c_int(), C.c_double()
    check(lib.mx_tonality_key(c, C.byref(k), C.byref(conf)))
    return k.value, conf.value


def video_scope_record_bytes(wave_cols: int = 0, vectorscope: bool = False) -> int:
    """bytes of one video scope record: 32 + 4 * (768 + 256 * wave_cols + 16384 * vectorscope) (host only, no device)"""
    n = C.c_size_t()
    check(lib.mx_video_scope_record_bytes(C.byref(VideoScopeParams(int(wave_cols), 1 if vectorscope else 0, 1)), C.byref(n)))
    return n.value


def parse_video_scope_records(raw: np.ndarray, wave_cols: int, vectorscope: bool) -> list:
    """raw bytes of back-to-back records -> one dict per record: the header fields as ints, hist [3, 256], wave [wave_cols, 256] or None,
    vec [128, 128] (indexed [V >> 1, U >> 1]) or None, all uint32"""
    words = video_scope_record_bytes(wave_cols, vectorscope) // 4
    r = np.ascontiguousarray(raw).view(np.uint32).reshape(-1, words)
    out = []
    for w in r:
        d = dict(zip(("present", "counted", "pixfmt", "width", "height", "tick_in_run"), (int(x) for x in w[:6])))
        d["reserved"] = (int(w[6]), int(w[7]))
        d["hist"] = w[8:776].reshape(3, 256)
        d["wave"] = w[776:776 + 256 * wave_cols].reshape(wave_cols, 256) if wave_cols else None
        d["vec"] = w[776 + 256 * wave_cols:].reshape(128, 128) if vectorscope else None
        out.append(d)
    return out


def log_band_edges(n_fft: int, n_bands: int, f_lo: float, f_hi: float, rate: float) -> np.ndarray:
    """n_bands + 1 strictly ascending bin indices (uint16) for mx_spectrum_params.edges: log-spaced between f_lo and f_hi Hz where the
    bins are dense enough, one bin per band below that.  Bin k is k * rate / n_fft Hz; the last edge is at most n_fft // 2 + 1."""
    top = n_fft // 2 + 1
    if not (0 < f_lo < f_hi and rate > 0 and 1 <= n_bands <= min(128, top)):
        raise ValueError("log_band_edges: need 0 < f_lo < f_hi, rate > 0 and 1 <= n_bands <= min(128, n_fft // 2 + 1)")
    f = f_lo * (f_hi / f_lo) ** (np.arange(n_bands + 1) / n_bands)
    e = np.clip(np.rint(f * n_fft / rate), 0, top).astype(np.int64)
    for j in range(1, n_bands + 1):          # at least one bin per band ...
        e[j] = max(e[j], e[j - 1] + 1)
    e[n_bands] = min(e[n_bands], top)
    for j in range(n_bands - 1, -1, -1):     # ... also where that pushed against the top
        e[j] = min(e[j], e[j + 1] - 1)
    return e.astype(np.uint16)


def check(rc: int) -> None:
    if rc != MX_OK:
        raise MxError(rc, (lib.mx_last_error() or b"").decode("utf-8", "replace"))


def params_bytes(p) -> bytes:
    """Serialise a params object (ctypes struct, list of MixerChannelParams, bytes or None)."""
    if p is None:
        return b""
    if isinstance(p, (bytes, bytearray)):
        return bytes(p)
    if isinstance(p, (list, tuple)):
        return b"".join(bytes(x) for x in p)
    return bytes(p)


def _graph_arrays(nodes, edges):
    """(mx_node[], mx_edge[], the buffers the node array points into) for a list of (kind, params) and of edge tuples."""
    keep = []
    n_arr = (Node * max(1, len(nodes)))()
    for i, (kind, p) in enumerate(nodes):
        blob = params_bytes(p)
        buf = C.create_string_buffer(blob, len(blob)) if blob else None
        keep.append(buf)
        n_arr[i] = Node(kind, len(blob), C.cast(buf, C.c_void_p) if buf else None)
    e_arr = (Edge * max(1, len(edges)))()
    for i, e in enumerate(edges):
        e_arr[i] = Edge(*e)
    return n_arr, e_arr, keep


def debug_plan(nodes, edges, sample_rate=44100, ticks_per_second=60, max_ticks_per_run=1, flags=0, overlap_auto=1, cap_frames=0):
    """mx_graph_debug_plan: (one PlanNode per node, PlanInfo) of the graph mx_graph_build would compile.  Needs no device; raises what a build raises."""
    n_arr, e_arr, _keep = _graph_arrays(nodes, edges)
    opts = GraphOpts(sample_rate, ticks_per_second, max_ticks_per_run, flags, -1, 0, None)
    out = (PlanNode * max(1, len(nodes)))()
    info = PlanInfo()
    check(lib.mx_graph_debug_plan(n_arr, len(nodes), e_arr, len(edges), C.byref(opts), overlap_auto, cap_frames, out, C.byref(info)))
    return list(out[: len(nodes)]), info


class Graph:
    """Thin RAII wrapper of mx_graph_* (a frozen Workspace, src/engine/workspace.rs:13-19)."""

    def __init__(self, nodes, edges, sample_rate=44100, ticks_per_second=60, max_ticks_per_run=1, flags=0,
                 device=-1, stream=None):
        self._h = C.c_void_p()
        n_arr, e_arr, self._keep = _graph_arrays(nodes, edges)
        opts = GraphOpts(sample_rate, ticks_per_second, max_ticks_per_run, flags, device, 0, stream)
        check(lib.mx_graph_build(n_arr, len(nodes), e_arr, len(edges), C.byref(opts), C.byref(self._h)))
        spt = C.c_size_t()
        check(lib.mx_graph_samples_per_tick(self._h, C.byref(spt)))
        self.spt = spt.value
        self.max_ticks = max_ticks_per_run
        self.n_nodes = len(nodes)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.mx_graph_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run_order(self):
        n = C.c_size_t()
        arr = (C.c_uint32 * max(1, self.n_nodes))()
        check(lib.mx_graph_run_order(self._h, arr, self.n_nodes, C.byref(n)))
        return list(arr[: n.value])

    def update_params(self, node, params):
        blob = params_bytes(params)
        check(lib.mx_graph_update_params(self._h, node, blob, len(blob)))

    def schedule_params(self, node, tick_in_run: int, params):
        """ModuleT::update at the boundary before tick `tick_in_run` of the next run (client_update between ticks)."""
        blob = params_bytes(params)
        check(lib.mx_graph_schedule_params(self._h, node, tick_in_run, blob, len(blob)))

    def schedule_params_batch(self, events: "C.Array", n: int | None = None):
        """events: a ctypes array of ParamEvent whose `params` pointers the caller keeps alive for the call."""
        check(lib.mx_graph_schedule_params_batch(self._h, events, len(events) if n is None else n))

    def eq_repair_stats(self) -> dict:
        """mx_graph_eq_repair_stats: what the proof / repair pass of the speculative EqThree did (counters since the graph was built)"""
        v = (C.c_uint64 * 8)()
        check(lib.mx_graph_eq_repair_stats(self._h, v))
        keys = ("chunks_run", "chunks_repaired", "settled_by_comparison", "walk_steps_16", "fill_steps_16", "island_rounds", "in_order_walks", "nan_fills")
        return {k: int(x) for k, x in zip(keys, v)}

    def debug_tail_releases(self):
        """-> (gated, at_once): how the held-back Mixer banks of the second-stream mode went out (mx_graph_debug_tail_releases)"""
        a, b = C.c_uint64(), C.c_uint64()
        check(lib.mx_graph_debug_tail_releases(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def debug_eq_launch(self) -> dict:
        """mx_graph_debug_eq_launch: the form the first EqThree group's last launch took -> {form: one of EQ_LAUNCH, super_block, n_chunks, chunk, warm}
        (the scan: n_chunks / chunk = the spans of its time split and their length, warm = what its pre-pass reads of each span; sequential:
        super_block = lanes per instance, 1 = one lane, 2 = the split cascade)"""
        v = (C.c_uint32 * 5)()
        check(lib.mx_graph_debug_eq_launch(self._h, v))
        return {"form": EQ_LAUNCH.get(v[0], str(v[0])), "super_block": int(v[1]), "n_chunks": int(v[2]), "chunk": int(v[3]), "warm": int(v[4])}

    def debug_eq_env_rows(self) -> bool:
        """mx_graph_debug_eq_env_rows: did some wave of the first EqThree group's last launch take the row form of the inline Envelope (synchronises)"""
        v = C.c_uint32()
        check(lib.mx_graph_debug_eq_env_rows(self._h, C.byref(v)))
        return bool(v.value)

    def debug_eq_lean(self) -> dict:
        """mx_graph_debug_eq_lean: did some wave of the first EqThree group's last launch run a tick without the input tracker / without the multiply by an
        amplitude of 1.0 (synchronises) -> {untracked, unity}"""
        v = C.c_uint32()
        check(lib.mx_graph_debug_eq_lean(self._h, C.byref(v)))
        return {"untracked": bool(v.value & 1), "unity": bool(v.value & 2)}

    def debug_eq_records(self):
        """-> (device pointer, bytes) of the first EqThree group's chunk records of the last speculative launch (mx_graph_debug_eq_records)"""
        p, n = C.c_void_p(), C.c_size_t()
        check(lib.mx_graph_debug_eq_records(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def eq_spec_stats(self):
        """-> (chunks run, chunks repaired) of the speculative exact EqThree path since the graph was built."""
        a, b = C.c_uint64(), C.c_uint64()
        check(lib.mx_graph_eq_spec_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def write_source(self, node, samples: np.ndarray, n_ticks: int):
        a = np.ascontiguousarray(samples, dtype=np.float32)
        check(lib.mx_graph_write_source(self._h, node, a.ctypes.data_as(C.c_void_p), n_ticks))

    def bind_source_device(self, node, device_ptr: int):
        check(lib.mx_graph_bind_source_device(self._h, node, C.c_void_p(device_ptr)))

    def run_ticks(self, first_tick: int, n_ticks: int = 1):
        check(lib.mx_graph_run_ticks(self._h, first_tick, n_ticks))

    def sync(self):
        check(lib.mx_graph_sync(self._h))

    def read_output(self, node, port, n_ticks: int, stereo: bool, rate=(1, 1)) -> np.ndarray:
        """rate = (up, down) of the port's sample-rate domain (a Resample node's output is not at the graph's rate)."""
        out = np.empty(n_ticks * (self.spt * rate[0] // rate[1]) * (2 if stereo else 1), dtype=np.float32)
        check(lib.mx_graph_read_output(self._h, node, port, out.ctypes.data_as(C.c_void_p), n_ticks))
        return out

    def read_output_window(self, node, port, first_tick: int, n_ticks: int, stereo: bool) -> np.ndarray:
        """ticks [first_tick, first_tick + n_ticks) of the last run (ports in the graph's own rate domain)"""
        out = np.empty(n_ticks * self.spt * (2 if stereo else 1), dtype=np.float32)
        check(lib.mx_graph_read_output_window(self._h, node, port, out.ctypes.data_as(C.c_void_p), first_tick, n_ticks))
        return out

    def read_audio_out(self, node, first_tick: int, n_ticks: int):
        """OutputDevice: (the floats pushed into the ring over ticks [first_tick, first_tick + n_ticks) of the last run, their per-tick records
        as a structured array of AUDIO_OUT_TICK_DTYPE)"""
        n = C.c_size_t(0)
        check(lib.mx_graph_read_audio_out(self._h, node, first_tick, n_ticks, None, 0, None, C.byref(n)))
        samples = np.empty(n.value, dtype=np.float32)
        ticks = np.empty(n_ticks, dtype=AUDIO_OUT_TICK_DTYPE)
        check(lib.mx_graph_read_audio_out(self._h, node, first_tick, n_ticks, samples.ctypes.data_as(C.c_void_p), n.value,
                                          ticks.ctypes.data_as(C.c_void_p), C.byref(n)))
        return samples, ticks

    def audio_out_lag(self, node):
        """the cpal callback ran short: the next run's first tick takes the note (any thread, also during a run)"""
        check(lib.mx_graph_audio_out_lag(self._h, node))

    def set_meters(self, ports, params=MeterParams(0, 1.0)):
        """level meters on output ports [(node, port), ...]; params: one MeterParams for every tap, or a list of one per tap.
        A tap already set keeps its peak-hold state; [] removes them all."""
        ports = list(ports)
        if isinstance(params, MeterParams):
            params = [params] * len(ports)
        pa = (PortRef * max(1, len(ports)))(*[PortRef(int(n), int(p)) for (n, p) in ports])
        pr = (MeterParams * max(1, len(ports)))(*[MeterParams(q.hold_ticks, q.release) for q in params])
        check(lib.mx_graph_set_meters(self._h, pa, len(ports), pr))
        self._n_meters = len(ports)

    def read_meters(self, first_tick: int, n_ticks: int) -> np.ndarray:
        """ticks [first_tick, first_tick + n_ticks) of the last run: a METER_TICK_DTYPE array shaped (n_ticks, taps) in set order"""
        n = getattr(self, "_n_meters", 0)
        out = np.zeros((n_ticks, n), dtype=METER_TICK_DTYPE)
        check(lib.mx_graph_read_meters(self._h, first_tick, n_ticks, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def set_spectra(self, ports, n_fft: int = 2048, edges=None):
        """spectrum taps on output ports [(node, port), ...]: every tick, the band powers of a Hann-windowed n_fft-point transform of the
        port's last n_fft frames.  edges: B + 1 ascending bin indices (log_band_edges makes them); one set for every tap.  Each call
        starts every tap from silence; [] removes them all."""
        ports = list(ports)
        if not ports:
            check(lib.mx_graph_set_spectra(self._h, None, 0, None))
            self._spectra = (0, 0)
            return
        e = np.ascontiguousarray(edges, dtype=np.uint16)
        if e.ndim != 1 or e.size < 2 or not np.array_equal(e, np.asarray(edges)):
            raise ValueError("edges: at least two bin indices that fit 16 bits")
        pa = (PortRef * len(ports))(*[PortRef(int(n), int(p)) for (n, p) in ports])
        pr = SpectrumParams(int(n_fft), e.size - 1, e.ctypes.data_as(C.POINTER(C.c_uint16)))
        check(lib.mx_graph_set_spectra(self._h, pa, len(ports), C.byref(pr)))
        self._spectra = (len(ports), e.size - 1)

    def read_spectra(self, first_tick: int, n_ticks: int) -> np.ndarray:
        """ticks [first_tick, first_tick + n_ticks) of the last run: float32 [ticks, taps in set order, channel, band]; 1.0 is a
        full-scale sine on a bin centre (10 * log10 of a value is its level in dB)"""
        n, b = getattr(self, "_spectra", (0, 0))
        out = np.zeros((n_ticks, n, 2, b), dtype=np.float32)
        check(lib.mx_graph_read_spectra(self._h, first_tick, n_ticks, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def set_loudness(self, ports, momentary_ticks: int = 24, short_ticks: int = 180):
        """loudness taps on output ports [(node, port), ...]: every tick, the K-weighted sum of squares per channel, its sums over the
        last momentary_ticks / short_ticks ticks and the true peak.  One window pair for every tap.  Each call starts every tap from
        silence; [] removes them all."""
        ports = list(ports)
        if not ports:
            check(lib.mx_graph_set_loudness(self._h, None, 0, None))
            self._n_loudness = 0
            return
        pa = (PortRef * len(ports))(*[PortRef(int(n), int(p)) for (n, p) in ports])
        check(lib.mx_graph_set_loudness(self._h, pa, len(ports), C.byref(LoudnessParams(int(momentary_ticks), int(short_ticks)))))
        self._n_loudness = len(ports)

    def read_loudness(self, first_tick: int, n_ticks: int) -> np.ndarray:
        """ticks [first_tick, first_tick + n_ticks) of the last run: a LOUDNESS_TICK_DTYPE array shaped (n_ticks, taps) in set order;
        lufs(rec["momentary_sq"], momentary_ticks * rec["frames"]) is the momentary loudness"""
        n = getattr(self, "_n_loudness", 0)
        out = np.zeros((n_ticks, n), dtype=LOUDNESS_TICK_DTYPE)
        check(lib.mx_graph_read_loudness(self._h, first_tick, n_ticks, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def set_stereo(self, ports, window_ticks: int = 180, grid: int = 0, zoom_log2: int = 0, hop: int = 1):
        """stereo field taps on stereo output ports [(node, port), ...]: every tick, the sums of L L, R R and L R and their sums over the last
        window_ticks ticks; with grid 64 or 128 a goniometer whose grid is emitted and cleared every hop ticks.  One parameter set for every
        tap.  Each call resets every tap and the hop counter; [] removes them all."""
        ports = list(ports)
        if not ports:
            check(lib.mx_graph_set_stereo(self._h, None, 0, None))
            self._stereo = (0, 0, 1)
            return
        pa = (PortRef * len(ports))(*[PortRef(int(n), int(p)) for (n, p) in ports])
        check(lib.mx_graph_set_stereo(self._h, pa, len(ports), C.byref(StereoParams(int(window_ticks), int(grid), int(zoom_log2), int(hop)))))
        self._stereo = (len(ports), int(grid), max(1, int(hop)))

    def read_stereo(self, first_tick: int, n_ticks: int) -> np.ndarray:
        """ticks [first_tick, first_tick + n_ticks) of the last run: a STEREO_TICK_DTYPE array shaped (n_ticks, taps) in set order;
        stereo_correlation(rec["win_ll"], rec["win_rr"], rec["win_lr"]) is the correlation meter's reading"""
        n = getattr(self, "_stereo", (0, 0, 1))[0]
        out = np.zeros((n_ticks, n), dtype=STEREO_TICK_DTYPE)
        check(lib.mx_graph_read_stereo(self._h, first_tick, n_ticks, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def read_goniometers(self) -> list:
        """the goniometer records the last run emitted: a list over its emissions of lists over the taps in set order of
        parse_goniometer_records dicts"""
        n, grid, hop = getattr(self, "_stereo", (0, 0, 1))
        rb = 32 + 4 * grid * grid
        raw = np.zeros(max(1, -(-self.max_ticks // hop)) * max(1, n) * rb, dtype=np.uint8)
        got = C.c_uint32()
        check(lib.mx_graph_read_goniometers(self._h, raw.ctypes.data_as(C.c_void_p), raw.size, C.byref(got)))
        recs = parse_goniometer_records(raw[: got.value * rb], grid)
        return [recs[i:i + n] for i in range(0, len(recs), n)] if n else []

    def set_limiters(self, ports, ceiling: float = 1.0, lookahead: int = 240):
        """look-ahead limiter taps on audio output ports [(node, port), ...]: every run writes a limited copy of each port, delayed by
        `lookahead` frames and never beyond +-ceiling, and one record per tick.  One parameter set for every tap.  Each call starts every
        tap's stream from silence; [] removes them all."""
        ports = list(ports)
        if not ports:
            check(lib.mx_graph_set_limiters(self._h, None, 0, None))
            self._n_limiters = 0
            return
        pa = (PortRef * len(ports))(*[PortRef(int(n), int(p)) for (n, p) in ports])
        check(lib.mx_graph_set_limiters(self._h, pa, len(ports), C.byref(LimiterParams(float(ceiling), int(lookahead)))))
        self._n_limiters = len(ports)

    def read_limiters(self, first_tick: int, n_ticks: int) -> np.ndarray:
        """ticks [first_tick, first_tick + n_ticks) of the last run: a LIMITER_TICK_DTYPE array shaped (n_ticks, taps) in set order"""
        n = getattr(self, "_n_limiters", 0)
        out = np.zeros((n_ticks, n), dtype=LIMITER_TICK_DTYPE)
        check(lib.mx_graph_read_limiters(self._h, first_tick, n_ticks, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def read_limited(self, tap: int, first_tick: int, n_ticks: int, i16: bool = False) -> np.ndarray:
        """the limited copy of tap `tap` (index in set order) over ticks [first_tick, first_tick + n_ticks) of the last run: float32 (or, with
        i16, the sinks' int16 format), frames x channels per tick, a stereo port interleaved"""
        n = C.c_size_t(0)
        check(lib.mx_graph_read_limited(self._h, tap, first_tick, n_ticks, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.int16 if i16 else np.float32)
        fn = lib.mx_graph_read_limited_i16 if i16 else lib.mx_graph_read_limited
        check(fn(self._h, tap, first_tick, n_ticks, out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)))
        return out

    def limited_device_ptr(self, tap: int):
        """-> (device pointer of tap `tap`'s limited copy of tick 0, floats from one tick's copy to the next)"""
        p, n = C.c_void_p(), C.c_size_t()
        check(lib.mx_graph_limited_device_ptr(self._h, tap, C.byref(p), C.byref(n)))
        return p.value, n.value

    def set_tempo(self, ports, hop_frames: int = 128, window_hops: int = 2048, max_lag: int = 512, emit_ticks: int = 6):
        """tempo taps on audio output ports [(node, port), ...]: every emit_ticks ticks one record per tap with the autocorrelation, over the
        last window_hops hops of hop_frames frames, of the port's onset function at lags 0 .. max_lag - 1 (tempo_bpm reads the tempo from
        it).  One parameter set for every tap.  Each call resets every tap and the emission counter; [] removes them all."""
        ports = list(ports)
        if not ports:
            check(lib.mx_graph_set_tempo(self._h, None, 0, None))
            self._tempo = (0, 16, 1)
            return
        pa = (PortRef * len(ports))(*[PortRef(int(n), int(p)) for (n, p) in ports])
        check(lib.mx_graph_set_tempo(self._h, pa, len(ports), C.byref(TempoParams(int(hop_frames), int(window_hops), int(max_lag), int(emit_ticks)))))
        self._tempo = (len(ports), int(max_lag), max(1, int(emit_ticks)))

    def read_tempo(self) -> list:
        """the tempo records the last run emitted: a list over its emissions of lists over the taps in set order of parse_tempo_records
        dicts"""
        n, max_lag, emit = getattr(self, "_tempo", (0, 16, 1))
        rb = 32 + 8 * max_lag
        raw = np.zeros(max(1, -(-self.max_ticks // emit)) * max(1, n) * rb, dtype=np.uint8)
        got = C.c_uint32()
        check(lib.mx_graph_read_tempo(self._h, raw.ctypes.data_as(C.c_void_p), raw.size, C.byref(got)))
        recs = parse_tempo_records(raw[: got.value * rb], max_lag)
        return [recs[i:i + n] for i in range(0, len(recs), n)] if n else []

    def set_tonality(self, ports, decim: int = 8, hop_frames: int = 512, octaves: int = 5, f_lo_mhz: int = 65406, emit_ticks: int = 30):
        """tonality taps on audio output ports [(node, port), ...]: every emit_ticks ticks one record per tap with, per constant-Q bin (12 per
        octave from f_lo_mhz up), the magnitudes of the hops completed since the previous record, summed; the analysis runs on the port's mid
        signal decimated by decim, a hop every hop_frames decimated frames (tonality_chroma and tonality_key read pitch classes and the key
        from the records).  One parameter set for every tap.  Each call resets every tap and the emission counter; [] removes them all."""
        ports = list(ports)
        if not ports:
            check(lib.mx_graph_set_tonality(self._h, None, 0, None))
            self._tonality = (0, 2, 1)
            return
        pa = (PortRef * len(ports))(*[PortRef(int(n), int(p)) for (n, p) in ports])
        par = TonalityParams(int(decim), int(hop_frames), int(octaves), int(f_lo_mhz), int(emit_ticks))
        check(lib.mx_graph_set_tonality(self._h, pa, len(ports), C.byref(par)))
        self._tonality = (len(ports), int(octaves), max(1, int(emit_ticks)))

    def read_tonality(self) -> list:
        """the tonality records the last run emitted: a list over its emissions of lists over the taps in set order of
        parse_tonality_records dicts"""
        n, octaves, emit = getattr(self, "_tonality", (0, 2, 1))
        rb = 32 + 96 * octaves
        raw = np.zeros(max(1, -(-self.max_ticks // emit)) * max(1, n) * rb, dtype=np.uint8)
        got = C.c_uint32()
        check(lib.mx_graph_read_tonality(self._h, raw.ctypes.data_as(C.c_void_p), raw.size, C.byref(got)))
        recs = parse_tonality_records(raw[: got.value * rb], octaves)
        return [recs[i:i + n] for i in range(0, len(recs), n)] if n else []

    def set_video_scopes(self, ports, wave_cols: int = 0, vectorscope: bool = False, hop: int = 1):
        """video scope taps on video output ports [(node, port), ...]: on every hop-th video tick, the luma / U / V histograms, the
        waveform's column histograms (wave_cols 0, 64, 128 or 256) and the vectorscope of the port's frame.  One parameter set for every
        tap; each call resets the hop counter; [] removes the taps."""
        ports = list(ports)
        if not ports:
            check(lib.mx_graph_set_video_scopes(self._h, None, 0, None))
            self._scopes = (0, 0, False, 1)
            return
        pa = (PortRef * len(ports))(*[PortRef(int(n), int(p)) for (n, p) in ports])
        pr = VideoScopeParams(int(wave_cols), 1 if vectorscope else 0, int(hop))
        check(lib.mx_graph_set_video_scopes(self._h, pa, len(ports), C.byref(pr)))
        self._scopes = (len(ports), int(wave_cols), bool(vectorscope), int(hop))

    def read_video_scopes(self) -> list:
        """the last run's records: a list over its recorded ticks of lists over the taps in set order of parse_video_scope_records dicts"""
        n, wave_cols, vec, hop = getattr(self, "_scopes", (0, 0, False, 1))
        rb = video_scope_record_bytes(wave_cols, vec)
        raw = np.zeros(max(1, -(-self.max_ticks // hop)) * max(1, n) * rb, dtype=np.uint8)
        got = C.c_uint32()
        check(lib.mx_graph_read_video_scopes(self._h, raw.ctypes.data_as(C.c_void_p), raw.size, C.byref(got)))
        recs = parse_video_scope_records(raw[: got.value * rb], wave_cols, vec)
        return [recs[i:i + n] for i in range(0, len(recs), n)] if n else []

    def read_output_i16(self, node, port, n_ticks: int, stereo: bool, rate=(1, 1)) -> np.ndarray:
        out = np.empty(n_ticks * (self.spt * rate[0] // rate[1]) * (2 if stereo else 1), dtype=np.int16)
        check(lib.mx_graph_read_output_i16(self._h, node, port, out.ctypes.data_as(C.c_void_p), n_ticks))
        return out

    def write_source_i16(self, node, samples: np.ndarray, n_ticks: int):
        a = np.ascontiguousarray(samples, dtype=np.int16)
        check(lib.mx_graph_write_source_i16(self._h, node, a.ctypes.data_as(C.c_void_p), n_ticks))

    def output_device_ptr(self, node, port):
        p = C.c_void_p()
        n = C.c_size_t()
        check(lib.mx_graph_output_device_ptr(self._h, node, port, C.byref(p), C.byref(n)))
        return p.value, n.value

    def stream(self):
        """the hipStream_t the graph launches on"""
        p = C.c_void_p()
        check(lib.mx_graph_stream(self._h, C.byref(p)))
        return p.value

    def tail_stream(self):
        """MX_FLAG_OVERLAP_TAIL: the stream the last launch group runs on (None when the mode is off)."""
        p = C.c_void_p()
        check(lib.mx_graph_tail_stream(self._h, C.byref(p)))
        return p.value

    def read_plotter(self, node, tick_in_run):
        l = np.empty(self.spt, dtype=np.float32)
        r = np.empty(self.spt, dtype=np.float32)
        fired = C.c_int()
        check(lib.mx_graph_read_plotter(self._h, node, tick_in_run, l.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), C.byref(fired)))
        return (l, r) if fired.value else None

    def profile_run(self, first_tick, n_ticks):
        by_kind = (C.c_float * PROFILE_KINDS)()
        total = C.c_float()
        check(lib.mx_graph_profile_run(self._h, first_tick, n_ticks, by_kind, C.byref(total)))
        return {KIND_NAMES[k]: by_kind[k] for k in range(PROFILE_KINDS) if by_kind[k] > 0}, total.value


    def profile_enable(self, on: bool):
        check(lib.mx_graph_profile_enable(self._h, 1 if on else 0))

    def profile_collect(self):
        """-> ({kind_name: total ms}, total ms, n_runs) accumulated since profile_enable(True)."""
        by_kind = (C.c_float * PROFILE_KINDS)()
        total = C.c_float()
        n = C.c_uint32()
        check(lib.mx_graph_profile_collect(self._h, by_kind, C.byref(total), C.byref(n)))
        return {KIND_NAMES[k]: by_kind[k] for k in range(PROFILE_KINDS) if by_kind[k] > 0}, total.value, n.value


    def performance_info(self, n_nodes: int):
        """-> (PerformanceInfo, [module us per tick]) for the most recent profiled run (src/engine/timing.rs:46-60)."""
        info = PerformanceInfo()
        us = (C.c_uint64 * max(1, n_nodes))()
        check(lib.mx_graph_performance_info(self._h, C.byref(info), us, n_nodes))
        return info, list(us[:n_nodes])

    def adopt_state(self, old: "Graph", old_node_of_new):
        """Topology edit (src/engine.rs:277-398): take over the state of surviving modules; `old` must not run again."""
        arr = (C.c_int32 * max(1, len(old_node_of_new)))(*old_node_of_new)
        check(lib.mx_graph_adopt_state(self._h, old._h, arr, len(old_node_of_new)))


class PcmRing:
    """mx_pcm_ring_*: decoded i16 frames of any length re-blocked to ticks (src/module/stream_input.rs:92-124)."""

    def __init__(self):
        self._h = C.c_void_p()
        check(lib.mx_pcm_ring_create(C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.mx_pcm_ring_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def push(self, samples: np.ndarray):
        a = np.ascontiguousarray(samples, dtype=np.int16)
        check(lib.mx_pcm_ring_push_i16(self._h, a.ctypes.data_as(C.c_void_p), a.size))

    def queued(self) -> int:
        n = C.c_size_t()
        check(lib.mx_pcm_ring_queued(self._h, C.byref(n)))
        return n.value

    def feed(self, graph: "Graph", node: int, n_ticks: int) -> int:
        z = C.c_size_t()
        check(lib.mx_pcm_ring_feed(self._h, graph._h, node, n_ticks, C.byref(z)))
        return z.value


class Module:
    """mx_module_*: one ModuleT instance with host buffers (src/module/mod.rs:7-19)."""

    def __init__(self, kind, params=None, sample_rate=44100, ticks_per_second=60, flags=0):
        self._h = C.c_void_p()
        blob = params_bytes(params)
        opts = GraphOpts(sample_rate, ticks_per_second, 1, flags, -1, 0, None)
        check(lib.mx_module_create_ex(kind, blob, len(blob), C.byref(opts), C.byref(self._h)))
        self.kind = kind

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.mx_module_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, params):
        blob = params_bytes(params)
        check(lib.mx_module_update(self._h, blob, len(blob)))

    def run_tick(self, t: int, inputs, outputs, indication: np.ndarray | None = None):
        """inputs: list of (line_kind, np.float32 array | None); outputs: list of (line_kind, np.float32 array)."""
        ins = (Input * max(1, len(inputs)))()
        keep = []
        for i, (lk, arr) in enumerate(inputs):
            if lk == MX_DISCONNECTED or arr is None:
                ins[i] = Input(MX_DISCONNECTED, None, 0, None)
            else:
                a = np.ascontiguousarray(arr, dtype=np.float32)
                keep.append(a)
                ins[i] = Input(lk, a.ctypes.data_as(C.c_void_p), a.size, None)
        outs = (Output * max(1, len(outputs)))()
        for i, (lk, arr) in enumerate(outputs):
            assert arr.dtype == np.float32 and arr.flags.c_contiguous
            outs[i] = Output(lk, arr.ctypes.data_as(C.c_void_p), arr.size, None, 0)
        ind_len = C.c_size_t(indication.nbytes if indication is not None else 0)   # in: capacity, out: bytes written
        ind_ptr = indication.ctypes.data_as(C.c_void_p) if indication is not None else None
        check(lib.mx_module_run_tick(self._h, t, ins, len(inputs), outs, len(outputs), ind_ptr, C.byref(ind_len)))
        return ind_len.value

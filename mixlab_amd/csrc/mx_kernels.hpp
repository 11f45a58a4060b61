// mx_kernels.hpp -- per-kind device descriptors and launcher prototypes (internal).
//
// One launch handles every instance of one module kind at one dependency level: instance = blockIdx.y
// (streaming kernels) or one wave / one lane (recurrences).  Descriptors are plain structs in device
// memory; all port buffers are raw device pointers into the graph's HBM slab (or caller-bound memory).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

namespace mx {

// src/module/amplifier.rs:38-60
struct AmpDesc { const float* in; const float* ctl; /* nullptr => Disconnected => mod 1.0 */ float* out; double amplitude; double mod_depth; };

// src/module/envelope.rs:34-58,91-120.  Reciprocals are loop-invariant subexpressions of the
// reference (`1.0 / params.attack_ms * ms`), evaluated once on the host with the same IEEE division.
struct EnvParams { double attack_ms, inv_attack, inv_decay, sustain, one_minus_sustain, inv_release; };
struct EnvDesc {
    const float* gate; float* out;
    float gate_const; uint32_t use_const;   // 1: gate is a Trigger fused in: constant 1.0 / 0.0, no buffer (trigger.rs:38-41)
                                            // 2: ... whose params change at tick boundaries inside this run: one bit per tick (GateBits)
    EnvParams p;
};
struct EnvState { uint32_t tag; uint32_t pad; uint64_t seq; double off_amplitude; };  // EnvelopeState, envelope.rs:8-13

// Per-tick parameter schedule of a Trigger (Engine::client_update between two ticks, src/engine.rs:192-214,277-398, applied
// inside one submission): bit c of an instance's row = gate_open during tick c of the run.  Rows are `words` u32 long,
// instance i of a launch group reads row i; `call_off` = first tick of this launch inside the run.
struct GateBits { const uint32_t* bits; uint32_t words; uint32_t call_off; };
__host__ __device__ inline bool gate_bit(const GateBits& g, uint32_t inst, uint32_t call) {
    const uint32_t c = g.call_off + call;
    return (g.bits[(size_t)inst * g.words + (c >> 5)] >> (c & 31)) & 1u;
}

// State of an Envelope whose gate is such a Trigger, as it ENTERS each tick of the run (k_env_ticks): with a gate that is
// constant over a tick only the tick's first sample can change the state (envelope.rs:99-115), so the EqThree kernels'
// fused epilogue reads one entry per tick and evaluates the closed form (envelope.rs:34-58) per sample from it.
//   flat: the amplitude no longer changes from this tick's first sample on (Initial, sustain reached, release finished):
//   `depth` = the Amplifier's depth() for that constant control (amplifier.rs:71-73), hoisted.
struct EnvTick { uint64_t seq; double off_amp; double depth; uint32_t tag; uint32_t flat; };
struct EnvTickDesc { EnvParams p; double amp_one_minus, amp_mod_depth; EnvState* state; };

// src/module/eq_three.rs:58-89
// epi: fused epilogue chosen by the graph compiler (mx_engine.cpp plan_fusion):
//   0  out[i] = y                                  (plain EqThree)
//   1  out[2i] = out[2i+1] = y                     (EqThree -> StereoPanner with L = R = this EQ)
//   2  out[2i] = out[2i+1] = amp(y, ctl[i])        (... -> Amplifier input; ctl nullptr => 1.0)
// y is the f32 the EQ would have stored, so the fused result is bit-identical to the three modules.
// MX_EQF_MONO_DUP: the stereo result has L == R by construction and every consumer is a Mixer input
//   that understands it, so ONE float per frame is stored (half the write, half the mixer's read).
// MX_EQF_ENV: the Amplifier's control is an Envelope whose gate is a Trigger constant and that feeds
//   nothing else: its closed-form amplitude (envelope.rs:34-58) is evaluated in the epilogue and the
//   control buffer never exists; env_state holds that Envelope's carried state.
enum { MX_EQF_MONO_DUP = 1u, MX_EQF_ENV = 2u };
struct EqDesc {
    const float* in; float* out; double gain_lo, gain_mid, gain_hi;
    const float* ctl; double amp_one_minus, amp_mod_depth, amp_amplitude; uint32_t epi; uint32_t flags;
    EnvParams env;   // MX_EQF_ENV: the folded Envelope's parameters; its per-tick states come from k_env_ticks (EnvTick table)
};
struct EqState { double lo[4]; double hi[4]; double history[3]; double pad; };       // eq_three.rs:13-26,100-103

// time-parallel EqThree: Toeplitz powers of the one-sample pole matrix, per chunk length L (host-computed)
//   pw[f][j] = first column of A_f^(L*j), j = 0..64 ; p2[f][k] = first column of A_f^(L * 2^k), k = 0..5
//   h[f][m]  = A_f^m b_f, m = 0..31 (impulse response of the 4 poles: phase A is 8 dot products against it)
//   cz[f]    = (sum_{m<L} A_f^m) c_f (what the VSA constant alone leaves in a zero-initialised filter after L samples)
struct EqScanTab { double pw[2][65][4]; double p2[2][6][4]; double h[2][32][4]; double cz[2][4]; };

// time-split plan of the scan kernel (see k_eq_three_scan MODE 1/2): wave-uniform kernel arguments
// warm / l2_pre: the pre-pass runs over the last `warm` samples of a span only (whole segments of 256 << l2_pre); see eq_plan_split
struct EqSplit { uint32_t n_split; uint32_t l2_pre; uint32_t stream_out /* outputs too large to stay cached: non-temporal stores */; uint32_t pad; size_t span; size_t warm; double* zbuf /* [n][n_split][8] */; double* bound /* [n][12] */; EnvState* env_snap /* [n] */; };
struct EqSpanPow { double lo[4], hi[4]; };   // first column of A^span per filter (host, long double)

// src/module/fm_sine.rs:37-56
struct FmDesc { const float* in; float* out; double freq_mid, freq_amp; };

// src/module/mixer.rs:46-71
struct MixChan { const float* in; double gain; /* fader * 10^(dB/20), mixer.rs:59 */ uint32_t cue; uint32_t dup; /* input stored as one float per frame (L == R) */ };
struct MixDesc { const MixChan* chans; uint32_t n_ch; uint32_t pad; float* master; float* cue; };

// src/module/oscillator.rs:65-92
struct OscDesc { float* mono; float* stereo; double freq; uint32_t waveform; uint32_t pad; };

// src/module/stereo_panner.rs:30-41 / stereo_splitter.rs:33-47
struct PanDesc { const float* l; const float* r; float* out; };
struct SplitDesc { const float* in; float* l; float* r; };

// src/module/trigger.rs:35-48
struct TrigDesc { float* out; float value; uint32_t pad; };   // a scheduled run reads GateBits instead of `value`

// src/module/plotter.rs:37-56: de-interleave the fired ticks into a staging area
struct PlotJob { const float* in; float* left; float* right; };

// build-specified FIR / rational resampler (mx_k_fir.hip); taps live in device memory, hist = carried input frames
struct FirDesc { const float* in; float* out; const double* taps; float2* hist; uint32_t n_taps; uint32_t pad; };
struct ResampleDesc { const float* in; float* out; const double* taps /* [up][taps_per_phase] */; float2* hist;
                      uint32_t up, down, taps_per_phase, pad; };

// Launchers.  `frames` = mono samples in this run (= n_ticks * SPT); stereo buffers hold 2*frames.
// fc (here and below): MX_FLAG_FP_CONTRACT -- the kernel instantiated for the contracted order (mul_add<true>, mx_env_math.hpp)
void launch_amplifier(const AmpDesc* d, uint32_t n, size_t frames, hipStream_t s, bool fc = false);
void launch_envelope(const EnvDesc* d, EnvState* st, uint32_t n, size_t frames, size_t fpc, const GateBits& gates, uint64_t t0, double sample_rate, hipStream_t s, bool fc = false,
                     void* scratch = nullptr, size_t scratch_bytes = 0 /* envelope_scratch_bytes(): segments of long streams (mx_k_envelope.hip); without it one wave per instance */);
size_t envelope_scratch_bytes(uint32_t n, size_t frames);
// per-tick Envelope states of the folded Envelopes of an EqThree group: ticks[inst][call], `n_calls` ticks of `fpc` samples from t0
void launch_env_ticks(const EnvTickDesc* d, uint32_t n, const GateBits& gates, uint32_t n_calls, size_t fpc, uint64_t t0, double sample_rate, EnvTick* ticks, hipStream_t s, bool fc = false);
// what every EqThree launch needs beyond the descriptors: the per-tick Envelope table (null when no instance folds one)
struct EqRun { size_t frames; size_t fpc /* samples per tick (call) */; uint32_t n_calls; uint32_t fc /* MX_FLAG_FP_CONTRACT: the contracted order */; uint64_t t0; double sr, rsr /* RN(1 / sr), host */, lo_f, hi_f; const EnvTick* ticks /* [n][n_calls] */;
               uint32_t* started = nullptr; uint32_t started_seq = 0; /* tiled speculative kernel: its last workgroup stores started_seq there when it starts (every earlier one has been placed by then): Graph's tail gate */
               uint32_t* env_rows = nullptr; uint32_t env_rows_seq = 0; /* tiled speculative kernel, row form of the inline Envelope: a wave that took it for some tick stores env_rows_seq there (mx_graph_debug_eq_env_rows); words 1 and 2 of the same line: a wave that ran some tick without the input tracker / without the multiply by an amplitude of 1.0 (mx_graph_debug_eq_lean) */
               uint32_t lean = 1; /* tiled speculative kernel, whole-tick inline Envelope: the lean forms of its hot loops where they are exact no-ops removed (0: MX_EQ_LEAN=0, A/B) */ };
// scratch != nullptr: the split-cascade form for few instances (eq_use_poles_split; eq_poles_scratch_bytes of scratch); else one lane per instance
void launch_eq_three_exact(const EqDesc* d, EqState* st, uint32_t n, const EqRun& r, void* scratch, hipStream_t s);
bool eq_use_poles_split(uint32_t n, size_t frames);
size_t eq_poles_scratch_bytes(uint32_t n, size_t frames);
int eq_scan_log2l(size_t frames);
void launch_eq_three_scan(const EqDesc* d, EqState* st, uint32_t n, const EqRun& r,
                          const EqScanTab* tabs /* 4 tables: L = 4, 8, 16, 32 */, const EqSplit& split, const EqSpanPow& pp, hipStream_t s);
// speculative time-parallel EXACT mode (k_eq_three_spec + k_eq_three_repair): see mx_k_eq_three.hip
struct EqSpecPlan { uint32_t n_chunks; uint32_t chunk; uint32_t warm; uint32_t pad; uint32_t warm_hi /* the high cascade runs over the last warm_hi samples of a warm-up only (tiled kernel) */; };
bool eq_plan_spec(uint32_t n, size_t frames, size_t fpc, double lo_f, double hi_f, EqSpecPlan& plan, bool whole_ticks = false /* an inline Envelope: chunks of whole ticks at any rate */,
                  bool two_tiles = false /* a control buffer: input and control tile per wave, ten waves per CU */);   // false: one lane per instance (launch_eq_three_exact)
size_t eq_spec_scratch_bytes(uint32_t n, const EqSpecPlan& plan);
// one wave that leaves when *flag has reached seq (or after limit_us): a launch queued behind it on its stream starts once the kernel that stores the flag has been placed
void launch_tail_gate(const uint32_t* flag, uint32_t seq, uint32_t limit_us, hipStream_t s);
int eq_epilogue_mode(uint32_t epi, uint32_t flags, bool has_ctl);   // 0..7: (epilogue kind) * 2 + (stereo store); the specialisation key
bool launch_eq_three_spec(const EqDesc* d, EqState* st, uint32_t n, const EqRun& r, const EqSpecPlan& plan, int uniform_mode /* 0..7, or -1: mixed */,
                          void* scratch, uint64_t* stats /* [2]: chunks run, chunks repaired */, hipStream_t s,
                          uint32_t* launch = nullptr /* [5]: what ran, as mx_graph_debug_eq_launch reports it (MX_EQ_LAUNCH_*, super-block, n_chunks, chunk, warm) */,
                          bool env_rows = true /* false (MX_EQ_ENV_ROWS=0, A/B): the inline Envelope keeps the lockstep form where the row form would be chosen */);
void eq_plan_split(uint32_t n, size_t frames, double lo_f, double hi_f, EqSplit& sp);
void launch_fm_sine(const FmDesc* d, uint32_t n, size_t frames, uint64_t t0, double sample_rate, hipStream_t s, int sin_mode /* mx_k_stream.hip SIN_MODE */);
void launch_mixer(const MixDesc* d, uint32_t n, uint32_t max_ch /* most channels of any mixer in the group */, size_t frames,
                  int dup_mode /* 0 none, 1 all, 2 mixed */, hipStream_t s);
void launch_oscillator(const OscDesc* d, uint32_t n, size_t frames, uint64_t t0, double sample_rate, hipStream_t s, int sin_mode);
void launch_panner(const PanDesc* d, uint32_t n, size_t frames, hipStream_t s);
void launch_splitter(const SplitDesc* d, uint32_t n, size_t frames, hipStream_t s);
void launch_trigger(const TrigDesc* d, uint32_t n, size_t frames, size_t fpc, const GateBits* gates /* null: constant per instance */, hipStream_t s);
void launch_plotter(const PlotJob* d, uint32_t n, size_t spt, hipStream_t s);
void launch_f32_to_i16(const float* in, int16_t* out, size_t n, int dup, hipStream_t s);
void launch_i16_to_f32(const int16_t* in, float* out, size_t n, hipStream_t s);
struct CopyJob { void* dst; const void* src; size_t bytes; };
void launch_copy_jobs(const CopyJob* device_jobs, uint32_t n, hipStream_t s);   // one block per job
// bytes out of page-locked host memory into device memory BY A KERNEL (the device reads the host buffer): ordered by the queue's own barrier packets like any launch
void launch_upload(void* dst_device, const void* src_pinned_host, size_t bytes, hipStream_t s);
// OutputDevice (src/module/output_device.rs:174-246, mx_k_out.hip): the node's state on the device (times in samples at the graph rate, -1 = None;
// statuses 0 None, 1 Recent, 2 Active) and one span's launch pair
struct OutState { int64_t last_clip, last_lag; uint32_t clip_status, lag_status; };
struct OutTick { uint8_t clip, clip_status, lag_status, changed; uint32_t channels; };   // = mx_audio_out_tick
struct OutRun {
    const float* in; uint32_t dup;          // the input port at the span's first tick; dup: stored as one float per frame (L == R)
    uint32_t frames, channels;              // frames per tick of the input's rate domain; the stream's channel count (0: no stream)
    int32_t left, right;                    // stored assignments (-1: None), already < channels
    uint32_t n_ticks;
    float* scratch; float* out;             // persistent scratch (frames * channels floats at least); the span's hand-off (n_ticks * frames * channels)
    uint32_t* partial;                      // n_ticks * out_route_blocks(frames, channels) clip partials
    OutState* state; OutTick* rec;          // device state; the span's per-tick records
    uint64_t t0; uint32_t spt, rate, lag;   // the span's first t (samples), samples per tick and rate of the graph; lag: the flag was set
};
uint32_t out_route_blocks(size_t frames_per_tick, uint32_t channels);
void launch_output_device(const OutRun& r, hipStream_t s);
// The audio tap sets (meters, spectrum, loudness, stereo field, limiter, tempo, tonality) read their ports through one descriptor per tap and buffer parity.
// Their run structs begin alike -- desc, n, n_ticks, stride -- and launch_taps is overloaded on them, so the engine splits and defers any of
// them the same way (TapSetOf::launch in mx_taps.hpp, Graph::launch_tap_set)
enum : uint32_t { METER_MONO = 0, METER_STEREO = 1, METER_DUP = 2 };   // METER_DUP: stereo stored as one float per frame (L == R)
struct TapDesc { const float* p; uint32_t frames, layout, slot, _pad; };   // p: the port at tick 0 of the run; layout: METER_*; slot: index in set order
// Level meters (mx_k_meter.hip, mixlab_gpu.h mx_graph_set_meters): the descriptor (TapDesc's first four fields, then the tap's own
// parameters), the per-tick record (= mx_meter_tick) and each channel's peak-hold state
struct MeterDesc { const float* p; uint32_t frames, layout, slot, hold_ticks; float release; uint32_t _pad; };
struct MeterTick { float peak[2], hold[2]; double sum_sq[2]; uint32_t over[2], frames, channels; };
struct MeterHold { float h; uint32_t a; };
struct MeterRun {
    const MeterDesc* desc; uint32_t n;       // the launch's taps
    uint32_t n_ticks, stride;                // ticks of the run; records per tick (every tap of the set)
    MeterTick* rec; MeterHold* state;        // rec[tick * stride + slot]; state[2 * slot + channel]
};
void launch_taps(const MeterRun& r, hipStream_t s);   // k_meter_reduce, then k_meter_hold
// Spectrum taps (mx_k_spectrum.hip, mixlab_gpu.h mx_graph_set_spectra): one descriptor per tap and buffer parity.  The history of a tap is
// the last n_fft frames of its stream before the run, in the port's own layout (one float per frame for mono / dup, two for stereo), kept
// in two buffers of 2 * n_fft floats each that alternate per run (hist[run parity][slot]).
struct SpecRun {
    const TapDesc* desc; uint32_t n;        // the launch's taps
    uint32_t n_ticks, stride;                // ticks of the run; taps of the whole set (records per tick)
    uint32_t n_fft, n_bands;
    const float* window; const float2* twiddle; const uint16_t* edges;   // device tables: n_fft, n_fft / 2, n_bands + 1
    const float* hist_in; float* hist_out;   // [slot][2 * n_fft]: read by this run, written for the next
    float* rec;                              // rec[((tick * stride + slot) * 2 + channel) * n_bands + band]
};
void launch_taps(const SpecRun& r, hipStream_t s);   // k_spectrum, then k_spectrum_history
// the tables of the spectrum spec, correctly rounded f32 (host only): window[n_fft], twiddle re / im [n_fft / 2]; false: n_fft is not a supported size
bool spectrum_tables(uint32_t n_fft, float* window, float* twiddle_re, float* twiddle_im);
// Loudness taps (mx_k_loudness.hip, mixlab_gpu.h mx_graph_set_loudness): one descriptor per tap and buffer parity, the per-tick record (=
// mx_loudness_tick) and per tap (slot) the coefficients of its own rate domain.  Carried per tap: the filter state of each channel, the last
// LOUD_HIST_TICKS ticks' ksq[0] + ksq[1] and the last LOUD_HIST_FRAMES frames of each channel; the two histories are kept twice and
// alternate per run like the spectrum taps' (read by this run, written for the next).
static constexpr uint32_t LOUD_HIST_TICKS = 1023, LOUD_HIST_FRAMES = 11, LOUD_MAX_FRAMES = 1u << 22;
struct LoudTick { double ksq[2], momentary_sq, short_sq; float true_peak[2]; uint32_t frames, channels; };
struct LoudCoef { double bq[10], carry[16]; };   // shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2; P[r][c] row-major
struct LoudRun {
    const TapDesc* desc; uint32_t n;        // the launch's taps
    uint32_t n_ticks, stride;                // ticks of the run; taps of the whole set (records per tick)
    uint32_t momentary_ticks, short_ticks;
    const LoudCoef* coef;                    // [slot]
    const float* interp;                     // [3][12]
    double* state;                           // [slot][channel][4]
    double* walk; uint32_t walk_ticks;       // [slot][channel][walk_ticks][4]: Z_k of the run's ticks, then their start states S_k
    const double* ehist_in; double* ehist_out;   // [slot][LOUD_HIST_TICKS]
    const float* xhist_in; float* xhist_out;     // [slot][channel][LOUD_HIST_FRAMES]
    LoudTick* rec;                           // rec[tick * stride + slot]
};
void launch_taps(const LoudRun& r, hipStream_t s);   // k_loud_peak; k_loud_zero, k_loud_scan, k_loud_energy (a one-tick run: one interleaved walk); k_loud_window
// the tables of the loudness spec (host only): biquads[10], carry[4][4] for a tick of `frames` frames, interp[3][12]; any may be null.
// false: rate is not finite or not above twice the shelf frequency, or frames is outside 1 .. LOUD_MAX_FRAMES
bool loudness_tables(double rate, uint32_t frames, double* biquads, double* carry, float* interp);
// Stereo field taps (mx_k_stereo.hip, mixlab_gpu.h mx_graph_set_stereo): one descriptor per tap and buffer parity and the per-tick record
// (= mx_stereo_tick).  Carried per tap: the last STEREO_HIST_TICKS ticks' three sums, kept twice and alternating per run like the loudness
// windows' history, and -- with a goniometer -- one grid in the shape of a record (8 header words of which [2] frames and [3] skipped are
// used, then grid x grid counts) that holds the ticks since the last emission.
static constexpr uint32_t STEREO_HIST_TICKS = 1023;
struct StereoTick { double sum_ll, sum_rr, sum_lr, win_ll, win_rr, win_lr; uint32_t frames, nonfinite; };
struct StereoRun {
    const TapDesc* desc; uint32_t n;         // the launch's taps (layout is METER_STEREO or METER_DUP)
    uint32_t n_ticks, stride;                // ticks of the run; taps of the whole set (records per tick)
    uint32_t window_ticks;
    const double* hist_in; double* hist_out; // [slot][STEREO_HIST_TICKS][3]: read by this run, written for the next
    StereoTick* rec;                         // rec[tick * stride + slot]
    // goniometer (grid = 0: none): tick t of the run belongs to group (phase + t) / hop; groups below n_emit are the run's records, the one
    // the run ends in stays in the carry grid
    uint32_t grid, zoom_log2, hop, phase;    // phase: the graph's counter c mod hop at the run's first tick
    uint32_t n_emit, rec_words;              // (phase + n_ticks) / hop; 8 + grid * grid
    uint32_t* gon_rec;                       // [emission][slot][rec_words]
    uint32_t* gon_carry;                     // [slot][rec_words]
};
inline size_t stereo_gonio_record_bytes(uint32_t grid) { return 32 + 4 * (size_t)grid * grid; }
void launch_taps(const StereoRun& r, hipStream_t s);   // k_stereo_emit (a run that emits), k_stereo_reduce, k_stereo_window
// Limiter taps (mx_k_limit.hip, mixlab_gpu.h mx_graph_set_limiters): the descriptor (TapDesc's first four fields, then the port's channels
// and where the tap's limited copy starts inside a tick of copies), the per-tick record (= mx_limiter_tick).  Carried per tap: the last
// 2 x lookahead frames of its stream as (L, R) pairs -- hist[slot][h] is the frame 2 x lookahead - h before the run's first -- kept twice and
// alternating per run like the spectrum taps' history.  LIMIT_TILE: frames of a run one workgroup limits.
static constexpr uint32_t LIMIT_MAX_LOOKAHEAD = 512, LIMIT_HIST_FRAMES = 2 * LIMIT_MAX_LOOKAHEAD, LIMIT_TILE = 2048, LIMIT_MAX_FRAMES = 1u << 30;
struct LimitDesc { const float* p; uint32_t frames, layout, slot, channels; uint64_t off; };
struct LimitTick { float min_gain, peak_out; uint32_t limited, nonfinite, frames, channels; };
struct LimitRun {
    const LimitDesc* desc; uint32_t n;       // the launch's taps
    uint32_t n_ticks, stride;                // ticks of the run; taps of the whole set (records per tick)
    float ceiling; uint32_t lookahead;
    const float* weights;                    // [lookahead + 1]
    const float2* hist_in; float2* hist_out; // [slot][LIMIT_HIST_FRAMES]: read by this run, written for the next
    float* out; size_t tick_floats;          // the copies: out[tick * tick_floats + desc.off + frame * channels + channel]
    LimitTick* rec;                          // rec[tick * stride + slot]
    uint32_t max_frames;                     // most frames per tick of any tap of the set
};
void launch_taps(const LimitRun& r, hipStream_t s);   // k_limit_init, then k_limit
// n_ticks rows of `width` floats, `pitch` floats apart, copied back to back (the staging of the limited copies' read-backs)
void launch_limit_gather(const float* src, size_t pitch, uint32_t width, uint32_t n_ticks, float* dst, hipStream_t s);
// the smoothing weights of the limiter spec, correctly rounded f32 (host only): w[lookahead + 1]; false: lookahead is above LIMIT_MAX_LOOKAHEAD
bool limiter_weights(uint32_t lookahead, float* w);
// Tempo taps (mx_k_tempo.hip, mixlab_gpu.h mx_graph_set_tempo): the descriptor (TapDesc's first four fields, then the stream position of the
// tap's port when the descriptors were uploaded: the run's first frame is pos0 + ticks0 x frames, from which every hop a run touches, every
// emission's last complete hop and hops_complete follow in integers).  Carried per tap: the energy of the hop in progress and A of the last
// complete hop (each kept twice, alternating per run like the onset history), the frames counted non-finite since the last emission, and the
// last W + L - 1 onsets.  The onsets live at the front of a linear array behind which a run appends those of the hops it completes, so every
// emission of the run reads one stretch of it; the array is kept twice and the run writes the next run's front out of place.
struct TempoDesc { const float* p; uint32_t frames, layout, slot, _pad; uint64_t pos0; };
struct TempoRun {
    const TempoDesc* desc; uint32_t n;       // the launch's taps
    uint32_t n_ticks, stride;                // ticks of the run; taps of the whole set (records per emission)
    uint32_t log2_hop, window_hops, max_lag, emit_ticks;
    uint32_t phase, n_emit;                  // the graph's counter c mod emit_ticks at the run's first tick; (phase + n_ticks) / emit_ticks
    uint64_t ticks0;                         // ticks since the descriptors were uploaded, before this run
    uint32_t max_touched, max_done;          // the most hops any tap's run touches / completes (grid sizes)
    uint32_t lin_stride, e_stride;           // words of one tap's linear array; hop energies of one tap
    uint32_t* lin; uint32_t* lin_next;       // [slot][lin_stride]: W + L - 1 carried onsets, then the run's; the next run's
    uint64_t* energy;                        // [slot][e_stride]: E of the hops this run completes
    const uint64_t* part_in; uint64_t* part_out;   // [slot]
    const uint32_t* amp_in; uint32_t* amp_out;     // [slot]
    uint32_t* nonfinite;                     // [slot]
    uint32_t* rec; uint32_t rec_words;       // rec[(emission * stride + slot) * rec_words]: 8 header words, then L uint64_t
};
inline size_t tempo_record_bytes(uint32_t max_lag) { return 32 + 8 * (size_t)max_lag; }
inline bool tempo_params_ok(uint32_t hop_frames, uint32_t window_hops, uint32_t max_lag, uint32_t emit_ticks) {
    return (hop_frames == 64 || hop_frames == 128 || hop_frames == 256) && window_hops >= 64 && window_hops <= 4096 && max_lag >= 16 && max_lag <= 1024 &&
           max_lag <= window_hops && emit_ticks >= 1;
}
// The lag rule of mx_tempo_bpm and mx_deck_beatgrid (host only): over R(0 .. L - 1) of an onset function hopped every `hop` frames, the candidate lags are the integers
// of [60 rate / (hop bpm_hi), 60 rate / (hop bpm_lo)] within [1, L - 2], `best` the first maximum of R over them and d the vertex of the parabola through R(best - 1),
// R(best), R(best + 1) where that one opens downwards, else 0.  false: R(0) = 0 or no candidate.  R returns double.
template <class RF>
inline bool tempo_lag(RF&& R, uint32_t L, uint32_t hop, double rate, double bpm_lo, double bpm_hi, uint32_t& best, double& d) {
    const double lo = std::max(1.0, std::ceil(60.0 * rate / ((double)hop * bpm_hi))), hi = std::min((double)(L - 2), std::floor(60.0 * rate / ((double)hop * bpm_lo)));
    if (R(0) == 0.0 || !(lo <= hi)) return false;
    best = (uint32_t)lo;
    for (uint32_t l = best + 1; l <= (uint32_t)hi; ++l)
        if (R(l) > R(best)) best = l;   // the first maximum
    const double den = R(best - 1) - 2.0 * R(best) + R(best + 1);
    d = den < 0.0 ? 0.5 * (R(best - 1) - R(best + 1)) / den : 0.0;
    return true;
}
void launch_taps(const TempoRun& r, hipStream_t s);   // k_tempo_emit (a run that emits), k_tempo_energy, k_tempo_onsets, k_tempo_acf (a run that emits)
// Tonality taps (mx_k_tonality.hip, mixlab_gpu.h mx_graph_set_tonality): the descriptor is TempoDesc's with the index of the tap's table set
// (one per rate domain of the set: f_b / fs_d depends on it) in place of the padding.  From pos0 + ticks0 x frames, the run's first frame,
// follow in integers the decimated frames a run completes (n D in [pos, end)), the hops among them and every emission's hop count.
// Carried per tap: the TON_QTAIL(D) newest quantised frames and the TON_DHIST(Hc) newest decimated frames (each at the front of an array kept
// twice, which a run reads and whose other copy it writes), the hops since the last emission (kept twice), and -- updated in place, by the
// tap's own threads and atomics only -- the sums C[b] and the non-finite frames since the last emission.
// A table set, at tab + index x tab_stride bytes: int16 fir[8 D] | uint32 len[B] | uint32 off[B] (pairs before bin b) | int16 kern[sum len][2].
struct TonDesc { const float* p; uint32_t frames, layout, slot, tab; uint64_t pos0; };
struct TonRun {
    const TonDesc* desc; uint32_t n;         // the launch's taps
    uint32_t n_ticks, stride;                // ticks of the run; taps of the whole set (records per emission)
    uint32_t log2_d, log2_hop, bins, emit_ticks, f_lo_mhz;
    uint32_t phase, n_emit;                  // the graph's counter c mod emit_ticks at the run's first tick; (phase + n_ticks) / emit_ticks
    uint64_t ticks0;                         // ticks since the descriptors were uploaded, before this run
    uint32_t max_groups, max_hops;           // the most stretches of D frames any tap's run holds / hops it completes (grid sizes)
    uint32_t lin_stride;                     // int16 of one tap's decimated array: TON_DHIST carried, then the run's
    const int16_t* qt; int16_t* qt_next;     // [slot][TON_QTAIL]
    int16_t* lin; int16_t* lin_next;         // [slot][lin_stride]
    const uint32_t* hops_in; uint32_t* hops_out;   // [slot]
    uint64_t* csum; uint32_t* nonfinite;     // [slot][bins]; [slot]
    const unsigned char* tab; uint32_t tab_stride;
    uint32_t* rec; uint32_t rec_words;       // rec[(emission * stride + slot) * rec_words]: 8 header words, then C[0 .. B) as uint64_t
};
constexpr uint32_t TON_Q = 17, TON_MAX_KERNEL = 2048;
inline uint32_t ton_qtail(uint32_t decim) { return 8 * decim - 1 + (decim - 1); }
inline uint32_t ton_dhist(uint32_t hop_frames) { return TON_MAX_KERNEL - 1 + hop_frames - 1; }
inline size_t tonality_record_bytes(uint32_t octaves) { return 32 + 8 * 12 * (size_t)octaves; }
inline bool tonality_params_ok(uint32_t decim, uint32_t hop_frames, uint32_t octaves, uint32_t f_lo_mhz, uint32_t emit_ticks) {
    return (decim == 4 || decim == 8) && (hop_frames == 128 || hop_frames == 256 || hop_frames == 512) && octaves >= 2 && octaves <= 6 && f_lo_mhz >= 1 &&
           emit_ticks >= 1;
}
// the tables of the spec in f64 on the host: fir[8 D], len[B], and -- kern not NULL -- kern[sum len][2]; *kern_pairs = sum len.  0: fine;
// 1: N_0 > 2048; 2: the top bin reaches 0.45 fs_d; 3: sum |c| > 65534; 4: rate is not finite and positive
int tonality_tables(double rate, uint32_t decim, uint32_t octaves, uint32_t f_lo_mhz, int16_t* fir, uint32_t* len, int16_t* kern, size_t* kern_pairs);
void launch_taps(const TonRun& r, hipStream_t s);   // k_ton_emit, k_ton_decimate, k_ton_cq (a run that completes a hop)
// Video scope taps (mx_k_scope.hip, mixlab_gpu.h mx_graph_set_video_scopes): ONE launch counts one frame into one record -- the 32-byte
// header, hist[3][256], wave[wave_cols][256], vec[128][128], all u32.  The counters of the record must be zero when the launch starts (the
// workgroups add their partial counts with integer atomics); the kernel writes the header itself.  counted = 0: header only.
struct ScopeArgs {
    const uint8_t* y; const uint8_t* u; const uint8_t* v;   // planes of a counted frame: 16-byte aligned, strides multiples of 16
    uint32_t y_stride, u_stride, v_stride;
    uint32_t width, height;                  // luma size; the chroma planes are (width >> 1) x (height >> 1)
    uint32_t wave_cols, vectorscope;         // mx_video_scope_params
    uint32_t present, counted, pixfmt, tick_in_run;   // header words
    uint32_t* rec;                           // the record (device)
};
inline size_t scope_record_bytes(uint32_t wave_cols, uint32_t vectorscope) { return 32 + 4 * ((size_t)768 + 256 * (size_t)wave_cols + (vectorscope ? 16384u : 0u)); }
void launch_video_scope(const ScopeArgs& a, hipStream_t s);

void launch_fir(const FirDesc* d, uint32_t n, uint32_t max_taps, size_t frames, hipStream_t s, bool fc = false);
void launch_resample(const ResampleDesc* d, uint32_t n, uint32_t max_taps, uint32_t tab_doubles /* max up * taps_per_phase */,
                     uint32_t win_frames /* max 255 * down / up + 2 + taps_per_phase */, size_t in_frames, size_t out_frames,
                     uint64_t in_base, uint64_t out_base, hipStream_t s, uint32_t common_up = 0 /* every channel's `up` when they all agree, else 0 */, bool fc = false,
                     uint32_t common_taps = 0, uint32_t common_down = 0 /* likewise taps_per_phase and `down` */);

// the deck's feed (mx_deck.hpp, mx_k_deck.hip): one launch over n decks x n_ticks ticks x ceil(spt / MX_DECK_CHUNK) chunks; tick t of deck i goes to decks[i].out + t * 2 * spt
struct DeckDev; struct DeckTickDev;
void launch_deck_feed(const DeckDev* decks, const DeckTickDev* ticks, const float* tables, uint32_t n, uint32_t n_ticks, uint32_t spt,
                      bool phase_varies /* some playing tick's lanes differ in phase: the kernel with the bank in LDS */, hipStream_t s);
// the key-locked decks of a feed (mx_deck.hpp, mx_k_deck_keylock.hip): the grain search, one workgroup per deck, then the render over n decks x n_ticks ticks x chunks
struct KlDeckDev; struct KlTickDev;
void launch_deck_keylock(const KlDeckDev* decks, const KlTickDev* ticks, const float* tables, uint32_t n, uint32_t n_ticks, uint32_t spt, hipStream_t s);
// the sweep filter of the decks of a feed that have one (mx_deck_filter.hpp, mx_k_deck_filter.hip), in place on their ports behind the two launches above and ahead of
// the echo: one wave per deck; ticks: n_ticks per deck
struct FilterDeckDev; struct FilterTickDev;
void launch_deck_filter(const FilterDeckDev* decks, const FilterTickDev* ticks, uint32_t n_decks, uint32_t n_ticks, uint32_t spt, hipStream_t s);
// the echo of the decks of a feed that have one (mx_deck_echo.hpp, mx_k_deck_echo.hip), in place on their ports behind the launches above: the first n_block decks
// in the one-block form (decks x ticks x chunks workgroups), the n_walk decks behind them in the sequential form (a workgroup per deck); ticks: n_ticks per deck
struct EchoDeckDev; struct EchoTickDev;
void launch_deck_echo(const EchoDeckDev* decks, const EchoTickDev* ticks, uint32_t n_block, uint32_t n_walk, uint32_t n_ticks, uint32_t spt, hipStream_t s);
// the reverb of the decks of a feed that have one (mx_deck_reverb.hpp, mx_k_deck_reverb.hip), in place on their ports behind all the launches above: a workgroup per
// deck walks its blocks; ticks: n_ticks per deck
struct ReverbDeckDev; struct ReverbTickDev;
void launch_deck_reverb(const ReverbDeckDev* decks, const ReverbTickDev* ticks, uint32_t n_decks, uint32_t n_ticks, uint32_t spt, hipStream_t s);
// the analysis of a deck's track (mx_deck_columns.hpp, mx_k_deck_analyse.hip): columns -> cols (n_cols x 56 bytes), their onsets -> cols and `onsets`, the autocorrelation -> R
// (max_lag words, zeroed here first); all on stream s.  The tap tables widened to int32 and padded with zeros travel as a kernel argument.  forms[DECK_AN_*]: what was
// launched (mx_deck_debug_last_analysis).  Settings the check passes, n_cols = ceil(n_frames / column).
struct DeckAnalyseTaps { int32_t lo[128], hi[128]; };
enum { DECK_AN_SEVERAL = 0, DECK_AN_TILED = 1, DECK_AN_SHORT = 2, DECK_AN_ONE = 3 };
void launch_deck_analyse(const uint32_t* track, uint64_t n_frames, uint32_t column, uint32_t K, uint32_t max_lag, const DeckAnalyseTaps& taps, void* cols, uint32_t* onsets,
                         uint64_t* R, uint64_t n_cols, uint32_t forms[4], hipStream_t s);
// the waveform picture of a deck's columns (mx_deck_waveform.hpp, mx_k_deck_waveform.hip): ceil(w / 64) workgroups, each a strip of 64 pixel columns over the full height
// of the three planes; every byte of a.plane[0 .. 3) is written once.  Settings the check passes; a.stride_y = 64 * ceil(w / 64), a.stride_c = a multiple of 64 >= w / 2.
struct WaveArgs;
void launch_deck_waveform(const WaveArgs& a, hipStream_t s);

}  // namespace mx

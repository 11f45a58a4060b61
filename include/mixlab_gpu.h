/*
 * mixlab_gpu.h -- C ABI of the MI355X-native tick engine for haileys/mixlab's per-tick module graph.
 *
 * The reference has no C ABI: modules are Rust types behind `trait ModuleT`
 * (src/module/mod.rs:7-19) dispatched through `DynModuleHostT` (src/engine/module.rs:88-94) by
 * `Engine::run_tick` (src/engine.rs:400-510).  This header is the thin extern-"C" surface a Rust
 * `GpuModule: ModuleT` adapter (or a replacement for Engine::run_tick's inner loop) binds with an
 * `extern "C"` block -- see INTEGRATION.md for the Rust side.  Plain pointers and sizes only.
 *
 * Error convention follows the reference's own extern-"C" boundary (FFmpeg I/O callbacks,
 * codec/src/ffmpeg.rs:25-26, codec/src/ffmpeg/ioctx.rs:51-67,136-152): never unwind across the
 * boundary, return a negative int sentinel, stash the message, let the caller fetch it
 * (mx_last_error) and re-raise on its side.
 *
 * Threading: like Engine::run_tick (one engine thread, src/engine.rs:78-93) a graph/module handle
 * is not re-entrant; different handles may be used from different threads.
 */
#ifndef MIXLAB_GPU_H
#define MIXLAB_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MX_ABI_VERSION 4u   /* 2: mx_exchange_*, mx_monitor_tick.dropped, mx_monitor_params_ex, packed RGB pixel formats; 3: MX_FLAG_FP_CONTRACT;
                              * 4: mx_graph_read_output_window, per-pixel alpha (MX_PIXFMT_YUVA420P, mx_dframe_*_alpha; the A byte of packed RGBA honoured);
                              *    later, without a bump (only additions): MX_KIND_OUTPUT_DEVICE, mx_graph_read_audio_out, mx_graph_audio_out_lag;
                              *    mx_port_ref, mx_meter_params, mx_meter_tick, mx_graph_set_meters, mx_graph_read_meters;
                              *    mx_spectrum_params, mx_graph_set_spectra, mx_graph_read_spectra, mx_spectrum_tables;
                              *    mx_video_scope_params, mx_graph_set_video_scopes, mx_graph_read_video_scopes, mx_video_scope_record_bytes, mx_video_scope;
                              *    mx_loudness_params, mx_loudness_tick, mx_graph_set_loudness, mx_graph_read_loudness, mx_loudness_tables, mx_loudness_gate;
                              *    mx_stereo_params, mx_stereo_tick, mx_graph_set_stereo, mx_graph_read_stereo, mx_graph_read_goniometers, mx_stereo_gonio_record_bytes,
                              *    mx_stereo_correlation;
                              *    mx_limiter_params, mx_limiter_tick, mx_graph_set_limiters, mx_graph_read_limiters, mx_graph_read_limited, mx_graph_read_limited_i16,
                              *    mx_graph_limited_device_ptr, mx_limiter_weights;
                              *    mx_tempo_params, mx_graph_set_tempo, mx_graph_read_tempo, mx_tempo_record_bytes, mx_tempo_bpm;
                              *    mx_tonality_params, mx_graph_set_tonality, mx_graph_read_tonality, mx_tonality_record_bytes, mx_tonality_tables, mx_tonality_chroma,
                              *    mx_tonality_key;
                              *    mx_multiview_view, mx_multiview_params, mx_multiview_status, mx_video_multiview, mx_graph_set_multiview, mx_graph_multiview_output;
                              *    mx_video_matte_params, mx_video_matte, mx_video_matte_check, mx_video_matte_wipe, mx_graph_set_video_source_matte;
                              *    mx_deck, mx_deck_params, mx_deck_head, mx_deck_tick, mx_deck_create, mx_deck_destroy, mx_deck_load_i16, mx_deck_set, mx_deck_seek,
                              *    mx_deck_schedule, mx_deck_check, mx_deck_plan, mx_deck_feed, mx_deck_read_ticks, mx_deck_state, mx_deck_step, mx_deck_tables,
                              *    mx_deck_debug_last_feed;
                              *    mx_deck_keylock, mx_deck_grain, mx_deck_set_keylock, mx_deck_keylock_check, mx_deck_keylock_search, mx_deck_grain_count, mx_deck_read_grains,
                              *    mx_deck_debug_last_keylock;
                              *    mx_deck_analysis, mx_deck_column, mx_deck_grid, mx_deck_analysis_check, mx_deck_analysis_bands, mx_deck_analyse, mx_deck_column_count,
                              *    mx_deck_read_columns, mx_deck_read_autocorr, mx_deck_columns_host, mx_deck_beatgrid, mx_deck_debug_last_analysis;
                              *    mx_plan_node, mx_plan_info, mx_graph_debug_plan;
                              *    mx_deck_tonality, mx_deck_tonality_check, mx_deck_tonality_count, mx_deck_analyse_tonality, mx_deck_read_tonality, mx_deck_tonality_host,
                              *    mx_deck_debug_last_tonality, mx_deck_loudness, mx_deck_loudness_check, mx_deck_loudness_count, mx_deck_analyse_loudness,
                              *    mx_deck_read_loudness, mx_deck_loudness_host, mx_deck_debug_last_loudness, mx_deck_loudness_gain, mx_tonality_camelot;
                              *    mx_deck_finegrid, mx_deck_comb, mx_deck_beats, mx_deck_fine_pick, mx_deck_sync_result, mx_deck_finegrid_check, mx_deck_finegrid_count,
                              *    mx_deck_finegrid_span, mx_deck_analyse_finegrid, mx_deck_read_finegrid, mx_deck_read_fine_onsets, mx_deck_finegrid_host,
                              *    mx_deck_finegrid_pick, mx_deck_finegrid_period, mx_deck_sync, mx_deck_debug_last_finegrid;
                              *    mx_deck_echo, mx_deck_set_echo, mx_deck_schedule_echo, mx_deck_echo_check, mx_deck_echo_delay, mx_deck_echo_state, mx_deck_echo_plan,
                              *    mx_deck_debug_last_echo;
                              *    mx_deck_filter, mx_deck_filter_carry, mx_deck_set_filter, mx_deck_schedule_filter, mx_deck_filter_check, mx_deck_filter_state,
                              *    mx_deck_read_filter_state, mx_deck_filter_design, mx_deck_filter_knob, mx_deck_filter_host, mx_deck_debug_last_filter;
                              *    mx_deck_reverb, mx_deck_reverb_carry, mx_deck_set_reverb, mx_deck_schedule_reverb, mx_deck_reverb_check, mx_deck_reverb_state,
                              *    mx_deck_read_reverb_lines, mx_deck_reverb_plan, mx_deck_reverb_host, mx_deck_reverb_design, mx_deck_debug_last_reverb;
                              *    mx_deck_bars, mx_deck_beat, mx_deck_bar_pick, mx_deck_bars_check, mx_deck_bars_count, mx_deck_bars_tables, mx_deck_analyse_bars,
                              *    mx_deck_read_bars, mx_deck_read_bar_folds, mx_deck_bars_host, mx_deck_bars_pick, mx_deck_grid_next, mx_deck_debug_last_bars;
                              *    mx_deck_tempomap, mx_deck_tempo_segment, mx_deck_tempomap_check, mx_deck_tempomap_count, mx_deck_tempomap_span, mx_deck_tempomap_host,
                              *    mx_deck_tempomap_path, mx_deck_tempomap_segments, mx_deck_tempomap_at, mx_deck_tempomap_step, mx_deck_analyse_tempomap,
                              *    mx_deck_read_tempomap, mx_deck_read_tempomap_onsets, mx_deck_debug_last_tempomap;
                              *    mx_wave_colour, mx_wave_grid, mx_wave_marker, mx_wave_range, mx_deck_waveform, mx_deck_waveform_check, mx_deck_waveform_view,
                              *    mx_deck_render_waveform, mx_deck_waveform_host, mx_deck_debug_last_waveform */

/* ---- status codes (0 ok, <0 error; cf. MIXLAB_IOCTX_ERROR / MIXLAB_IOCTX_PANIC) ---- */
enum {
    MX_OK = 0,
    MX_ERR_INVALID = -1,  /* bad argument / id out of range */
    MX_ERR_TYPE = -2,     /* port line-type mismatch: the reference panics (src/engine/io.rs:40-41,49-50) or refuses the connection (src/engine/workspace.rs:97-114) */
    MX_ERR_DEVICE = -3,   /* HIP runtime error */
    MX_ERR_NOMEM = -4,
    MX_ERR_INTERNAL = -5, /* C++ exception caught at the boundary ("panic") */
    MX_ERR_FULL = -6      /* a bounded ingest queue is full: where the reference's sender blocks (sync_channel) or gets Err (ring push) */
};

/* ---- line types: protocol LineType, src/engine/io.rs:19-24 ---- */
typedef enum { MX_DISCONNECTED = 0, MX_MONO = 1, MX_STEREO = 2, MX_VIDEO = 3 } mx_line;

/* ---- module kinds: the DSP members of enumerate_modules! (src/module/mod.rs:27-49) ---- */
enum {
    MX_KIND_AMPLIFIER = 0,        /* src/module/amplifier.rs       in: Stereo, Mono(control)  out: Stereo */
    MX_KIND_ENVELOPE = 1,         /* src/module/envelope.rs        in: Mono(gate)             out: Mono */
    MX_KIND_EQ_THREE = 2,         /* src/module/eq_three.rs        in: Mono                   out: Mono */
    MX_KIND_FM_SINE = 3,          /* src/module/fm_sine.rs         in: Mono                   out: Stereo */
    MX_KIND_MIXER = 4,            /* src/module/mixer.rs           in: Stereo x N             out: Stereo Master, Stereo Cue */
    MX_KIND_OSCILLATOR = 5,       /* src/module/oscillator.rs      in: -                      out: Mono, Stereo */
    MX_KIND_PLOTTER = 6,          /* src/module/plotter.rs         in: Stereo                 out: - (indication) */
    MX_KIND_STEREO_PANNER = 7,    /* src/module/stereo_panner.rs   in: Mono L, Mono R         out: Stereo */
    MX_KIND_STEREO_SPLITTER = 8,  /* src/module/stereo_splitter.rs in: Stereo                 out: Mono L, Mono R */
    MX_KIND_TRIGGER = 9,          /* src/module/trigger.rs         in: -                      out: Mono */
    MX_KIND_VIDEO_MIXER = 10,     /* src/module/video_mixer.rs     in: Video x 4              out: Video Output, A, B */
    MX_KIND_SOURCE_MONO = 11,     /* host/device-fed port; stands in for the audio outputs of the I/O modules */
    MX_KIND_SOURCE_STEREO = 12,   /*   (StreamInput src/module/stream_input.rs:72-147, MediaSource media_source.rs:93-126) */
    MX_KIND_SOURCE_VIDEO = 13,    /* frame-fed port; stands in for MediaSource / StreamInput video (media_source.rs:93-126) */
    MX_KIND_VIDEO_TO_RGBA = 14,   /* BUILD-SPECIFIED sink (no reference module): YUV420P -> RGBA8 (+ Q12 3x4 matrix)  in: Video */
    MX_KIND_FIR = 15,             /* BUILD-SPECIFIED (BASELINE configs[2]; no reference module): K-tap FIR on a stereo stream  in: Stereo  out: Stereo */
    MX_KIND_RESAMPLE = 16,        /* BUILD-SPECIFIED rational polyphase resampler (44.1 -> 48 kHz = up 160 / down 147; the reference has only
                                     `TODO implement resampling`, src/icecast/mod.rs:94-97)  in: Stereo  out: Stereo at rate * up / down */
    MX_KIND_MONITOR = 17,         /* the hand-off of Monitor / StreamOutput (src/module/monitor.rs:113-139, stream_output.rs:154-158) and the first steps of
                                     their codec threads (monitor.rs:226-236; encode.rs:183-195 f32->i16, :287-295 DynamicScaler to the
                                     encoder's picture): keeps every tick's program frame, scaled, and serves the mix as i16
                                     in: Video, Stereo  out: --   params: mx_monitor_params */
    MX_KIND_OUTPUT_DEVICE = 18,   /* src/module/output_device.rs: the sound-card sink's tick-thread work -- routing into the device's interleaved frame, clip test,
                                     Clip / Lag indication (run_tick :174-246); cpal and its ring stay on the host.  in: Stereo  out: --
                                     params: mx_output_device_params; read with mx_graph_read_audio_out */
    MX_KIND_COUNT = 19
};
/* mx_graph_profile_run / _collect write this many per-kind times (the kinds that have launch groups of their own; an OutputDevice's time shows in
 * ms_total and in mx_graph_performance_info's module_us) */
#define MX_PROFILE_KINDS 18

/* protocol/src/lib.rs:233-241, bincode variant order */
enum { MX_WAVE_ON = 0, MX_WAVE_OFF = 1, MX_WAVE_SINE = 2, MX_WAVE_SQUARE = 3, MX_WAVE_TRIANGLE = 4, MX_WAVE_SAW = 5 };

/* ---- parameter structs: #[repr(C)] mirrors of protocol/src/lib.rs ---- */
typedef struct { double gain_db; double fader; uint8_t cue; uint8_t _pad[7]; } mx_mixer_channel_params; /* MixerChannelParams :342-347; MixerParams = array of these (params_len / sizeof) :329-332 */
typedef struct { double gain_lo_db, gain_mid_db, gain_hi_db; } mx_eq_three_params;                     /* EqThreeParams :285-290 (Decibel = f64 dB :455-456) */
typedef struct { double attack_ms, decay_ms, sustain_amplitude, release_ms; } mx_envelope_params;      /* EnvelopeParams :310-316 */
typedef struct { double amplitude, mod_depth; } mx_amplifier_params;                                   /* AmplifierParams :298-302 */
typedef struct { double freq; uint32_t waveform; uint32_t _pad; } mx_oscillator_params;                /* OscillatorParams :243-247 */
typedef struct { double freq_lo, freq_hi; } mx_fm_sine_params;                                         /* FmSineParams :292-296 */
typedef struct { uint32_t gate_open; } mx_trigger_params;                                              /* GateState :304-308 */
typedef struct { int32_t a, b; /* -1 = None */ double fader; } mx_video_mixer_params;                  /* VideoMixerParams :405-410 */
typedef struct { int32_t use_matrix; int32_t matrix_q12[12]; } mx_video_to_rgba_params;                /* build-specified, DESIGN.md "Colour" */
typedef struct { uint32_t width, height; } mx_monitor_params;   /* the encoder's picture: 560 x 350 (monitor.rs:21-22), 1120 x 700 (stream_output.rs:23-24); even */
/* The same with the reference's back-pressure (opt-in; params_len selects the form).  Monitor / StreamOutput hand every tick to their codec
 * thread with try_send on a channel of TWO and DROP the tick when it is full (monitor.rs:163-177, stream_output.rs:316-320).  queue_depth > 0:
 * the node holds at most that many ticks the consumer has not taken (mx_graph_monitor_consume); a tick that finds the queue full is dropped --
 * no picture is scaled or kept, mx_monitor_tick.dropped = 1 -- exactly what the codec thread would never see.  queue_depth = 0 (and the short
 * form): every tick of a submission is kept (one scaled frame per tick stays on the device until the next run: max_ticks_per_run x frame bytes). */
typedef struct { uint32_t width, height, queue_depth, _pad; } mx_monitor_params_ex;
/* OutputDeviceParams (protocol) as the adapter sees it once cpal has opened the stream: channels = the open stream's config.channels, 0 = no
 * stream (no device, or not found: output_device.rs:95-150); left / right = the requested channel, -1 = None.  channels <= 256, left / right
 * >= -1 (else MX_ERR_INVALID).  Creation applies them as the first update from the empty state; every update (output_device.rs:152-169) with
 * a stream open zeroes the whole scratch when the STORED left / right (already filtered) differ from the requested ones, then stores
 * left / right filtered by < channels; with channels = 0 the stored left / right are kept and nothing is zeroed. */
typedef struct { uint32_t channels; int32_t left, right; uint32_t _pad; } mx_output_device_params;
/* Build-specified audio extras (DESIGN.md "FIR and resampler").  Both are variable-length blobs: the header below
 * followed by the f64 coefficients.  Arithmetic: f32 widened to f64, accumulated in f64 in ascending tap index with
 * separate multiply and add, rounded once to f32 -- the reference's own convention (mixer.rs:62, amplifier.rs:56). */
/* mx_fir_params: 1 <= n_taps <= 16384.  A launch group (the Fir nodes of one dependency level) whose longest filter keeps the tiled kernel's LDS plan within
 * 64 KiB -- up to 1605 taps -- runs tiled (k_fir<8> from 8192 frames per run on and up to 1024 taps, else k_fir<4>); a group with a longer filter takes the plain
 * kernel for all its members (one output per lane, taps and frames from memory).  Same sums, same bits. */
typedef struct { uint32_t n_taps; uint32_t _pad; /* double taps[n_taps] */ } mx_fir_params;               /* y[n] = sum_k taps[k] x[n-k] per channel */
typedef struct { uint32_t up, down, taps_per_phase, _pad; /* double taps[up][taps_per_phase] */ } mx_resample_params;
/*   output sample M (absolute): n = floor(M * down / up), phase = (M * down) mod up, y[M] = sum_k taps[phase][k] x[n-k].
 *   A node's output lives in the sample-rate domain (rate * up / down); modules whose arithmetic depends on the sample
 *   rate or on t (EqThree, Envelope, Oscillator, FmSine) are only accepted in the base domain. */

/* ---- graph description ---- */
typedef struct { uint32_t kind; uint32_t params_len; const void* params; } mx_node;
typedef struct { uint32_t src_node, src_port, dst_node, dst_port; } mx_edge;  /* workspace.connections: InputId -> OutputId */

/* EqThree arithmetic.  DEFAULT: bit-exact with the reference's sequential order (src/module/eq_three.rs:58-89) -- the
 * reference's own module test asserts exact equality with its golden file (eq_three.rs:150-167) and the default passes it.
 * MX_FLAG_EQ_FAST opts into the time-parallel chunked scan: NOT bit-exact -- every f32 output is within 1 ULP of the
 * reference order and about 1 sample in 20 000 differs (DESIGN.md "EqThree").  MX_FLAG_EQ_EXACT is the default's old
 * name, kept as a no-op; it wins if both are given. */
#define MX_FLAG_EQ_EXACT 1u
#define MX_FLAG_EQ_FAST 4u
/* MX_FLAG_FP_CONTRACT: the CONTRACTED order -- the reference's f64 expressions with every multiply fused into the add that consumes
 * it (what -ffp-contract=fast makes of the same source; Rust itself never contracts).  It applies to EqThree
 * (p += f * (in - p) as fma(f, in - p, p), pole 0's + VSA as fma(f, in - p, VSA), the band mix as fma(hi, g_hi, fma(mid, g_mid, lo * g_lo)),
 * eq_three.rs:76-88,117-124), Envelope (sustain + (1 - sustain) * decay as one fma, envelope.rs:46-47), Amplifier (depth() as one fma,
 * amplifier.rs:71-73) and the build-specified Fir / Resample (acc = fma(h[k], x, acc), ascending k).  NOT bit-exact with the
 * reference: every f32 output is within 1 ULP of the exact order's (26 instead of 36 f64 instructions per EqThree sample).  The
 * contracted order is as deterministic as the exact one -- speculation, proof and repair work on it unchanged -- and the oracle's
 * contract mode (orc_set_fp_contract) restates it, so it is tested bit for bit.  Not with MX_FLAG_EQ_FAST (the scan has its own
 * arithmetic): mx_graph_build fails with MX_ERR_INVALID. */
#define MX_FLAG_FP_CONTRACT 16u

#define MX_FLAG_OVERLAP_TAIL 8u /* throughput mode for batched runs: the Mixer groups at the END of the launch order (a bank, or a bank and the
                                  group / master buses above it) run on a second stream beside the NEXT run's earlier groups (an HBM-bound kernel beside a VALU-bound one); the ports it
                                  reads are double-buffered and alternate per run.  Results are unchanged bit for bit; mx_graph_sync, every
                                  read-back and mx_graph_run_ticks' own ordering cover both streams.  mx_graph_output_device_ptr of a port
                                  the tail READS names the buffer of the last run only (it alternates); the tail's own outputs do not move.
                                  The bank's launch of run k is HELD BACK until run k + 1 has queued its EqThree launch (it then starts once that launch's
                                  workgroups are placed) or until something joins the two streams: mx_graph_sync, any read-back, an exchange's submit, a run cut
                                  by a scheduled update, and mx_graph_tail_stream() itself.  A consumer on another stream of the tail's outputs therefore calls
                                  mx_graph_tail_stream() AFTER the run it wants and orders itself after the stream it returns.
                                  WITHOUT the flag the library takes this mode on its own for graphs with at least 64 EqThree instances built for submissions of
                                  at least 16 ticks (runs of fewer ticks stay on one stream), while the second buffers fit (MX_OVERLAP_AUTO_MAX_GB, default 32, and
                                  a quarter of the free device memory) and only while no HOST holds a raw pointer the mode would not keep fresh:
                                  mx_graph_output_device_ptr of one of the tail's outputs, or of a port the tail reads (double-buffered in this mode), ends the
                                  automatism for that graph for good -- everything outstanding completes, the last run's data is where the pointer says, and from
                                  then on the graph is a one-stream graph (stream-ordered consumers see one-stream ordering as before).  An mx_exchange over a bus
                                  does NOT end it: the exchange orders itself behind the bank on whichever stream it runs.  1024 strips x 2048 ticks: 5.3 -> 4.8 ms per run.
                                  MX_OVERLAP_AUTO=0 (environment) turns it off. */
#define MX_FLAG_NO_FUSE 2u   /* materialise every port.  By default the graph compiler folds EqThree -> StereoPanner(L = R)
                                [-> Amplifier [<- Envelope <- Trigger]] into the EQ kernel, a single-consumer Trigger into
                                its Envelope, and stores an L == R stereo result that only Mixers read as one float per
                                frame.  Folded ports are per-tick temporaries (src/engine.rs:461,504-506) and cannot be
                                read back.  Results on every remaining port are bit-identical either way. */

typedef struct {
    uint32_t sample_rate;        /* 0 => 44100 (src/engine.rs:53) */
    uint32_t ticks_per_second;   /* 0 => 60    (src/engine.rs:54) */
    uint32_t max_ticks_per_run;  /* 0 => 1; port buffers hold this many consecutive ticks */
    uint32_t flags;              /* MX_FLAG_* */
    int32_t device;              /* HIP device ordinal, -1 => current */
    int32_t _pad;
    void* stream;                /* hipStream_t to launch on; NULL => the graph creates its own */
} mx_graph_opts;

typedef struct mx_graph mx_graph;

/* Thread-local message for the last failing call on this thread (ioctx "stash then report"). */
const char* mx_last_error(void);
uint32_t mx_abi_version(void);
/* Number of visible HIP devices, or <0. */
int mx_device_count(void);

/* Freeze a topology (the state Engine::run_tick reads from Workspace, src/engine/workspace.rs:13-19)
 * and allocate every port buffer in one HBM slab.  Connections are type-checked like
 * Workspace::connect (workspace.rs:97-114): mismatch => MX_ERR_TYPE. */
int mx_graph_build(const mx_node* nodes, size_t n_nodes, const mx_edge* edges, size_t n_edges,
                   const mx_graph_opts* opts, mx_graph** out);
void mx_graph_destroy(mx_graph* g);

int mx_graph_samples_per_tick(const mx_graph* g, size_t* spt);                 /* SAMPLES_PER_TICK, src/engine.rs:55 */
int mx_graph_run_order(const mx_graph* g, uint32_t* order, size_t cap, size_t* n); /* DFS order of src/engine.rs:421-457 */

/* The hipStream_t the graph launches on (the one given in mx_graph_opts, or its own): for ordering other device work against a run. */
int mx_graph_stream(mx_graph* g, void** stream);
/* MX_FLAG_OVERLAP_TAIL (or the automatic mode): the stream the last launch group runs on (NULL when the mode is off or the graph has no such group).
 * Releases a launch of that group the library was holding back for the next run (see the flag): call it after the run whose result is wanted. */
int mx_graph_tail_stream(mx_graph* g, void** stream);

/* ModuleT::update (src/module/mod.rs:16): replace one node's params between ticks. */
int mx_graph_update_params(mx_graph* g, uint32_t node, const void* params, size_t params_len);

/* Engine::client_update BETWEEN two ticks of one submission (src/engine.rs:192-214 drains the command queue after every tick;
 * :277-398 applies ModuleT::update): `params` replace `node`'s at the boundary before tick `tick_in_run` (0-based) of the NEXT
 * mx_graph_run_ticks, which must cover that tick (else that run fails with MX_ERR_INVALID and drops its schedule).  Updates for
 * the same node and tick apply in submission order; after the run the node holds the last one.  A Trigger's updates cost nothing
 * (one gate bit per tick read by the kernels that folded it in); an update of any other kind cuts the run into separately
 * launched spans at its tick.  The _batch form queues many at once (one foreign call per run). */
typedef struct { uint32_t node; uint32_t tick_in_run; const void* params; size_t params_len; } mx_param_event;
int mx_graph_schedule_params(mx_graph* g, uint32_t node, uint32_t tick_in_run, const void* params, size_t params_len);
int mx_graph_schedule_params_batch(mx_graph* g, const mx_param_event* events, size_t n_events);

/* Counters of the default EqThree path on long streams (speculative time-parallel form proven bit-exact chunk by chunk,
 * DESIGN.md "EqThree"), accumulated since the graph was built: stream chunks run, and chunks whose start state the
 * verification pass found different from the sequential order's and re-ran (exactly-constant input after a signal).
 * Synchronises the graph's stream. */
int mx_graph_eq_spec_stats(mx_graph* g, uint64_t* chunks_run, uint64_t* chunks_repaired);
/* The same counters with what the proof / repair pass did about them: out[0] chunks run, [1] chunks not proven by their recorded start
 * state, [2] of those settled by comparing outputs under a constant input (O(1)), [3] walk steps of 16 samples (both trajectories re-run
 * side by side, outputs rewritten), [4] fill steps of 16 samples (constant input, standing state, outputs differ), [5] rounds of islands
 * walked side by side, [6] in-order walks after an island that ended apart from the speculative run, [7] streams finished by the NaN fill. */
int mx_graph_eq_repair_stats(mx_graph* g, uint64_t out[8]);
/* DEBUG / profiling aid: the chunk records of the first EqThree launch group's last speculative launch (device memory owned by the graph, valid until the next run;
 * synchronises).  144 bytes per chunk: start[8], end[8] (f64 poles), min / max input bits, and in the padding -- written by the tiled kernel -- lane 0 of a wave: the
 * shader clock (low 32 bits) when the wave entered, lane 1: HW_ID, lane 2: XCC_ID, every lane: the clock when it left.  tools/wave_times.py reads it. */
int mx_graph_debug_eq_records(mx_graph* g, void** device_records, size_t* bytes);
/* DEBUG: how the Mixer banks of the second-stream mode (MX_FLAG_OVERLAP_TAIL / automatic) went out since the graph was built: behind the gate that the next run's EqThree
 * launch opens, or at once (a join released them, or the next run had no such launch).  Tests use it to know which path they exercised. */
int mx_graph_debug_tail_releases(mx_graph* g, uint64_t* gated, uint64_t* at_once);
/* DEBUG: which form the first EqThree launch group's last launch took (MX_EQ_LAUNCH_NONE before any).  out[0] the form, out[1] the super-block of a tiled
 * form -- 16 (half lines, two tiles), 32 (whole lines, two tiles) or 321 (whole lines, one tile) -- else 0 (sequential: see below), out[2] chunks per instance, out[3] the chunk
 * length in samples, out[4] the warm-up of a speculative chunk.  The scan form: out[2] the spans of its time split, out[3] the span length, out[4] the
 * samples its pre-pass reads at the end of each span (the span itself: the full pre-pass).  The sequential form: 1 chunk of the whole stream, no warm-up, and out[1] the
 * lanes per instance: 1 (one lane walks the stream) or 2 (the split cascade: a lane per 4-pole cascade and a sample-parallel epilogue kernel).
 * Tests use it to know which path a sample rate and tick length reached. */
#define MX_EQ_LAUNCH_NONE 0u
#define MX_EQ_LAUNCH_SEQUENTIAL 1u     /* one lane (or the two-lane split cascade) per instance, no speculation */
#define MX_EQ_LAUNCH_DIRECT 2u         /* speculative chunks, k_eq_three_spec (no tile) */
#define MX_EQ_LAUNCH_TILED 3u          /* speculative chunks, tiled kernel, chunks and ticks whole super-blocks */
#define MX_EQ_LAUNCH_RAGGED_TICK 4u    /* speculative chunks, tiled kernel for an inline Envelope whose ticks are not whole 32-sample super-blocks */
#define MX_EQ_LAUNCH_CONTROL_TILE 5u   /* speculative chunks, tiled kernel with a control tile (an Amplifier modulated by a buffer) */
#define MX_EQ_LAUNCH_SCAN 6u           /* MX_FLAG_EQ_FAST: the time-parallel scan */
int mx_graph_debug_eq_launch(mx_graph* g, uint32_t out[5]);
/* DEBUG: *rows = 1 if some wave of the first EqThree launch group's last launch evaluated its inline Envelope in the ROW form (the tiled kernel, at most two waves per
 * SIMD: a control tile the wave fills itself, ramping rows evaluated row by row), else 0 -- another form was launched (MX_EQ_ENV_ROWS=0, three or four waves per SIMD,
 * ragged ticks, no inline Envelope), or no tick of any wave had a ramping row beside none of the general form.  Synchronises.  Tests use it to know the row form ran. */
int mx_graph_debug_eq_env_rows(mx_graph* g, uint32_t* rows);
/* DEBUG: *lean = bit 0: some wave of the first EqThree launch group's last launch ran a tick of its whole-tick inline Envelope loops WITHOUT the input tracker (every lane of
 * the wave had seen two different input patterns in its chunk by then); bit 1: some wave ran them without the multiply by an amplitude of exactly 1.0.  0: MX_EQ_LEAN=0,
 * another form was launched, or no tick qualified.  Synchronises.  Tests use it to know the lean loops ran. */
int mx_graph_debug_eq_lean(mx_graph* g, uint32_t* lean);
/* DEBUG: what the graph compiler decides about a topology, WITHOUT a device: the run order, levels, sample-rate domains, the fusion plan, the launch groups, the
 * overlap-tail candidate and the slab layout, computed by the very code mx_graph_build runs before it opens the device.  Invalid graphs get the codes and messages
 * mx_graph_build gives them.  overlap_auto: what the environment's MX_OVERLAP_AUTO would say (0: the automatic second-stream mode off); cap_frames: frames per run
 * the slab is laid out for (0: samples per tick * max_ticks_per_run).  The tail candidate is reported as the compiler names it and the layout gives its ports their
 * second buffers; whether a build takes an AUTOMATIC candidate also depends on the device memory that is free then.  nodes_out: one record per node; info may be NULL. */
typedef struct mx_plan_node {
    int32_t pos;                  /* position in the run order; -1: outside it */
    int32_t level, group;         /* dependency level; launch group (-1: none -- elided, an OutputDevice, or outside the run order) */
    uint32_t slot;                /* index inside the group */
    int32_t sub_key;              /* EqThree: 1 + the epilogue mode its group is specialised for; 0 otherwise */
    uint32_t dom_num, dom_den, in_dom_num, in_dom_den;   /* sample-rate domain of the outputs / the inputs, relative to the graph's rate */
    uint32_t elided;              /* 1: never launched, its work is folded into `owner`'s kernel */
    int32_t owner;                /* -1: none */
    int32_t fuse_pan, fuse_amp, fuse_trigger, fuse_env;   /* the nodes folded into this one (-1: none) */
    uint32_t n_out;               /* output ports (at most 4) */
    uint8_t out_elided[4];        /* per output port: no buffer */
    uint8_t out_dup[4];           /* per output port: stereo with L == R stored as one float per frame */
    uint64_t out_off[4];          /* per output port: offset of its buffer in the slab, in floats; UINT64_MAX: none */
    uint64_t out_off2[4];         /* ... of its second buffer (a port the overlap tail reads); UINT64_MAX: none */
} mx_plan_node;
typedef struct mx_plan_info {
    uint64_t n_order, n_groups;   /* nodes in the run order; launch groups */
    uint64_t slab_floats;         /* the whole slab */
    uint64_t zero_off, zero_floats;   /* the region Disconnected inputs read */
    int32_t tail_first_group;     /* overlap-tail candidate: its first group (every later group belongs to it); -1: none */
    uint32_t tail_ports;          /* ... the output ports it would double-buffer */
    uint32_t tail_auto;           /* ... 1: by the automatic rule, 0: asked for with MX_FLAG_OVERLAP_TAIL */
    uint32_t has_video;
} mx_plan_info;
int mx_graph_debug_plan(const mx_node* nodes, size_t n_nodes, const mx_edge* edges, size_t n_edges, const mx_graph_opts* opts,
                        uint32_t overlap_auto, size_t cap_frames, mx_plan_node* nodes_out, mx_plan_info* info);

/* Feed a SOURCE_* node: n_ticks consecutive tick buffers (SPT mono / 2*SPT interleaved stereo f32). */
int mx_graph_write_source(mx_graph* g, uint32_t node, const float* host_samples, size_t n_ticks);
/* Or bind an external device buffer holding max_ticks_per_run tick buffers (read-only, caller-owned). */
int mx_graph_bind_source_device(mx_graph* g, uint32_t node, const void* device_ptr);

/* n_ticks consecutive Engine::run_tick calls (src/engine.rs:400-510) in one submission:
 * tick k of the run uses t = (first_tick + k) * SPT (src/engine.rs:490).  Asynchronous on the
 * graph's stream.  n_ticks <= max_ticks_per_run.  first_tick need not continue the previous run's: the clock may start anywhere and
 * jump between runs (carried state such as an Envelope's last edge keeps its absolute sample time); tested for sample times up to 2^40
 * and for Envelope distances of 2^32 samples and more (tests/test_gpu_far_clock.py). */
int mx_graph_run_ticks(mx_graph* g, uint64_t first_tick, uint32_t n_ticks);
int mx_graph_sync(mx_graph* g);

/* Copy an output port's buffers of the last run to the host (synchronises the stream). */
int mx_graph_read_output(mx_graph* g, uint32_t node, uint32_t port, float* host_samples, size_t n_ticks);
/* The same for ticks [first_tick_in_run, first_tick_in_run + n_ticks) of the last run only: a consumer that wants the tail of a long
 * submission (or a checker that samples it) does not pay PCIe for the rest. */
int mx_graph_read_output_window(mx_graph* g, uint32_t node, uint32_t port, float* host_samples, size_t first_tick_in_run, size_t n_ticks);
/* The data formats either side of the path, converted on the device so PCIe carries 2 bytes per sample:
 *   sinks (Monitor / StreamOutput, src/video/encode.rs:183-195): clamp to [-1, 1], * 32767.0, `as i16` (saturating, truncating);
 *   ingest (StreamInput, src/module/stream_input.rs:167-173):    sample as f32 / 32768.0. */
int mx_graph_read_output_i16(mx_graph* g, uint32_t node, uint32_t port, int16_t* host_samples, size_t n_ticks);
int mx_graph_write_source_i16(mx_graph* g, uint32_t node, const int16_t* host_samples, size_t n_ticks);

/* Device pointer + per-tick length (floats) of an output port (for zero-copy consumers / RCCL). */
int mx_graph_output_device_ptr(mx_graph* g, uint32_t node, uint32_t port, void** device_ptr, size_t* floats_per_tick);

/* MX_KIND_OUTPUT_DEVICE after a run: ticks [first_tick_in_run, first_tick_in_run + n_ticks) of the last mx_graph_run_ticks.
 *   samples  what run_tick would have pushed into the cpal ring over those ticks (stream.tx.push_slice, output_device.rs:210), concatenated in
 *            tick order: frames * channels floats per tick (frames = the input's samples per tick in its own rate domain), nothing for a tick
 *            with no stream.  Positions of no assigned channel hold the scratch as it was: zeros after a reassignment, stale samples of an
 *            earlier layout after a change of channel count.
 *   ticks    one record per tick: clip (a written sample was < -1 or > 1), clip_status / lag_status (0 None, 1 Recent, 2 Active -- the
 *            encoding of mx_performance_info.lag), changed (the reference's run_tick returned Some: a status differs from the previous
 *            tick's), channels.
 *   Clock: the graph's own -- tick k's `now` is its t in samples; Active when (now - last) * 10 < sample_rate (100 ms), Recent when now - last
 *   < 5 * sample_rate (5 s).  At 44 100 / 60 and 48 000 / 60 a clip stays Active for 6 ticks (the 6th later tick is exactly 100 ms: not
 *   Active) and Recent until 300 ticks later.  The node assumes the tick count only moves forward, as the reference's Instant does: after a
 *   run whose first tick lies BEFORE a recorded clip or lag, now - last is negative and reads as Active (signed arithmetic) until the
 *   clock has passed that time by 100 ms.
 * samples or ticks may be NULL (not copied); *n_samples (may be NULL) receives the float count of the window, and with both NULL the call is
 * a size query only.  samples_cap < that count, a window beyond the last run or a node of another kind: MX_ERR_INVALID.  Joins the graph's
 * streams like mx_graph_read_output. */
typedef struct { uint8_t clip, clip_status, lag_status, changed; uint32_t channels; } mx_audio_out_tick;
int mx_graph_read_audio_out(mx_graph* g, uint32_t node, uint32_t first_tick_in_run, uint32_t n_ticks, float* samples, size_t samples_cap,
                            mx_audio_out_tick* ticks, size_t* n_samples);
/* The cpal data callback ran short (output_device.rs:117-129, the store at :126): sets the node's lag flag.  Safe to call from any thread, concurrently with
 * mx_graph_run_ticks; the first tick of the next run consumes it (lag_flag.swap(false), :219). */
int mx_graph_audio_out_lag(mx_graph* g, uint32_t node);
/* mx_graph_adopt_state and an OutputDevice: the module persists across a topology edit, so the new node takes the old one's STATE as the
 * reference's module keeps it -- channel count, stored (filtered) left / right, scratch, clip / lag times and statuses, a pending lag note --
 * and the params it was built with are not applied.  A host that changed something at the same time (another device, another channel
 * count or assignment) applies it afterwards with mx_graph_update_params, exactly as OutputDevice::update would have seen it. */

/* Level meters: taps on output ports of a built graph.  A tap observes a port: it is no module, adds no edge and changes
 * neither the run order nor the fusion plan.  Every run measures each tap's every tick on the device, once per run after its last span:
 *   peak      the largest |x| of the tick per channel: the integer maximum of bits(x) & 0x7fffffff, read as f32 (a NaN shows as the largest
 *             NaN pattern of the tick, +Inf as +Inf)
 *   sum_sq    sum of x*x in f64 in a fixed order: 64 partials, partial j adds (double)x * (double)x of the frames f = j (mod 64) in ascending f
 *             from +0.0, then s[j] = s[j] + s[j ^ k] for k = 32, 16, 8, 4, 2, 1; the result is s[0].  mean square = sum_sq / frames
 *   over      samples with x < -1 or x > 1 (OutputDevice's clip test; NaN and +-1.0 do not count)
 *   hold      per channel h (f32) and age a (u32), both 0 when the tap is set; every tick in order: a = min(a + 1, UINT32_MAX); when
 *             a > hold_ticks, h = isfinite(h) ? h * release : 0; when bits(peak) >= bits(h), h = peak and a = 0; record h.  Carried across runs.
 *   frames    frames of the tick in the port's own rate domain (a Resample output has rate * up / down); channels: 1 mono, 2 stereo (for a mono
 *             port every [1] field is 0).  A stereo port stored as one float per frame (the fused L == R strip result) meters both channels
 *             from that float: the records equal MX_FLAG_NO_FUSE's bit for bit. */
typedef struct { uint32_t node, port; } mx_port_ref;
typedef struct { uint32_t hold_ticks; float release; } mx_meter_params;   /* release: finite, 0 < release <= 1 */
typedef struct {
    float    peak[2];
    float    hold[2];
    double   sum_sq[2];
    uint32_t over[2];
    uint32_t frames;
    uint32_t channels;
} mx_meter_tick;   /* 48 bytes: peak 0, hold 8, sum_sq 16, over 32, frames 40, channels 44 */
/* Replaces the graph's taps with ports[0..n), params[i] for ports[i] (n = 0: none; the graph then launches nothing for meters).  Video port:
 * MX_ERR_TYPE.  A node or port out of range, a duplicate (node, port), bad params, or a port the fusion did not materialise: MX_ERR_INVALID.
 * Waits for outstanding work like a read-back but keeps the automatic second-stream mode on.  A tap whose (node, port) was in the previous
 * set keeps its hold state; a new one starts from 0.  Device memory: max_ticks_per_run x n x 48 bytes of records + 8 bytes per channel.
 * mx_graph_adopt_state does not carry taps: set them again on the new graph.  Meter launches count in the profile calls' ms_total only. */
int mx_graph_set_meters(mx_graph* g, const mx_port_ref* ports, size_t n, const mx_meter_params* params);
/* Ticks [first_tick_in_run, first_tick_in_run + n_ticks) of the last run, laid out [tick][tap] in set order; cap = records dst holds.
 * A window beyond the last run (or a run made before the taps were set), cap < n_ticks x taps, or no taps: MX_ERR_INVALID.  Joins the
 * graph's streams like mx_graph_read_output. */
int mx_graph_read_meters(mx_graph* g, uint32_t first_tick_in_run, uint32_t n_ticks, mx_meter_tick* dst, size_t cap);

/* Spectrum analyser taps on output ports of a built graph.  Like a meter, a tap observes a port: no module, no edge, the
 * run order and the fusion plan unchanged; a graph without them launches nothing new.  Meters and spectrum taps are independent sets and may be
 * set together.  Every run computes, on the device and once per run after its last span, for each tap, tick t and channel the band powers of
 * a windowed n_fft-point transform.  The numbers are fixed bit for bit (tests/spectrum_model.py restates them in numpy):
 *   frame     the last N = n_fft frames of the port's stream that end with tick t's last frame, in the port's own rate domain (a Resample
 *             output has rate * up / down frames per tick).  Frames before the call to mx_graph_set_spectra read as +0.0; the history is
 *             carried across ticks and runs.  Every call to mx_graph_set_spectra resets every tap's history (no tap survives it, unlike a meter's hold).
 *   tables    window[i] = the f32 nearest to 0.5 - 0.5 cos(2 pi i / N) (periodic Hann); twiddle[k] = the f32s nearest to cos(2 pi k / N) and
 *             -sin(2 pi k / N), k < N / 2.  mx_spectrum_tables returns the very tables the kernels use.
 *   transform z[i] = (x_L[i] * window[i], x_R[i] * window[i]) as (re, im), f32 products; a mono port has im = +0.0.  Then the radix-2
 *             decimation-in-time data flow on bit-reversed input: log2 N stages s = 0 .., half-size h = 2^s; for every block start b (a
 *             multiple of 2h) and k < h: w = twiddle[k * N / (2h)], t = (z[b+k+h].re*w.re - z[b+k+h].im*w.im, z[b+k+h].re*w.im + z[b+k+h].im*w.re),
 *             z[b+k+h] = z[b+k] - t, z[b+k] = z[b+k] + t.  Every f32 operation is rounded on its own (no fused multiply-add); the multiply
 *             is performed for every twiddle, w = 1 included; subnormals are kept.
 *   split     bins k = 0 .. N/2, n = (N - k) mod N:  L = (Z[k].re + Z[n].re, Z[k].im - Z[n].im), R = (Z[k].im + Z[n].im, Z[n].re - Z[k].re) in f32
 *   power     p[k] = (double)c.re * (double)c.re + (double)c.im * (double)c.im: exact products, one f64 rounding
 *   band j    bins edges[j] <= k < edges[j+1]: 64 f64 partials, partial q adds the p[k] with (k - edges[j]) mod 64 == q in ascending k from
 *             +0.0, then s[q] = s[q] + s[q ^ m] for m = 32, 16, 8, 4, 2, 1 (the meters' order); the value is (float)(s[0] * (4.0 / ((double)N * N))).
 *             The scale is a power of two, hence exact; with it a full-scale sine on a bin centre reads 1.0 (0 dB) in a band of that one
 *             bin: the window sums to N / 2, so the bin's amplitude is N / 4, the split (which drops its halves) doubles it, and
 *             (N / 2)^2 * 4 / N^2 = 1.  The window also puts a quarter of that into each neighbouring bin: a band that holds all three reads 1.5.
 * A mono port's [1][*] is 0.  A stereo port stored as one float per frame (the fused L == R strip result) gives both channels from that
 * float, equal to MX_FLAG_NO_FUSE's records bit for bit.  Non-finite input makes bands NaN or Inf.
 * Accuracy: both channels travel through one complex transform, so the rounding error of the louder channel leaks into the quieter one.
 * Against an f64 transform, |sqrt(band) - sqrt(f64 band)| <= (6.66 log2 N + 4) * 2^-24 * sqrt(the f64 power of BOTH channels over all bins):
 * a channel far more than 120 dB below the other reads the other's rounding floor, not its own spectrum.
 * One parameter set holds for every tap of the graph (params points at ONE mx_spectrum_params).  edges are bin indices chosen by the
 * caller (bin k is k * rate / n_fft Hz): the library evaluates no transcendental for them. */
typedef struct {
    uint32_t        n_fft;     /* 256, 512, 1024, 2048 or 4096 */
    uint32_t        n_bands;   /* B: 1 .. 128 */
    const uint16_t* edges;     /* B + 1 bin indices, strictly ascending, edges[B] <= n_fft / 2 + 1; read during the call only */
} mx_spectrum_params;
/* Replaces the graph's spectrum taps with ports[0..n) (n = 0: none; params may then be NULL and the graph launches nothing for them).
 * Video port: MX_ERR_TYPE.  A node or port out of range, a duplicate (node, port), a port the fusion did not materialise, an n_fft, n_bands
 * or edges outside the above: MX_ERR_INVALID.  Waits for outstanding work like a read-back but keeps the automatic second-stream mode on.
 * Device memory: max_ticks_per_run x n x 2 x B floats of records + 4 x n_fft floats of history per tap.  mx_graph_adopt_state does not carry
 * taps: set them again on the new graph.  The launches count in the profile calls' ms_total only (MX_PROFILE_KINDS is unchanged).  The
 * per-module path (mx_module_*) exposes no graph handle, so taps cannot be set there. */
int mx_graph_set_spectra(mx_graph* g, const mx_port_ref* ports, size_t n, const mx_spectrum_params* params);
/* Ticks [first_tick_in_run, first_tick_in_run + n_ticks) of the last run as floats [tick][tap in set order][channel 0, 1][B]; cap = floats
 * dst holds.  A window beyond the last run (or a run made before the taps were set), cap < n_ticks x taps x 2 x B, or no taps:
 * MX_ERR_INVALID.  Joins the graph's streams like mx_graph_read_output. */
int mx_graph_read_spectra(mx_graph* g, uint32_t first_tick_in_run, uint32_t n_ticks, float* dst, size_t cap);
/* The tables of the spec for one n_fft: window[n_fft], twiddle_re[n_fft / 2], twiddle_im[n_fft / 2] (any of them may be NULL).  Host only:
 * touches no device and needs no graph.  Another n_fft: MX_ERR_INVALID. */
int mx_spectrum_tables(uint32_t n_fft, float* window, float* twiddle_re, float* twiddle_im);

/* Loudness taps on output ports of a built graph: per tick the K-weighted energy of ITU-R BS.1770-4 / EBU R 128 with its
 * momentary and short-term window sums, and the true peak.  Like a meter, a tap observes a port: no module, no edge, the run order and the
 * fusion plan unchanged; a graph without them launches nothing new.  Meters, spectrum taps and loudness taps are independent sets and may be
 * set together.  Every run computes the records on the device, once per run after its last span.  The numbers are fixed bit for bit
 * (tests/loudness_model.py restates them in numpy); every f64 operation is rounded on its own (no fused multiply-add):
 *   biquads   computed on the host in f64 from the port's own rate (a Resample output has rate * up / down).  Shelf: f0 = 1681.974450955533,
 *             G = 3.999843853973347 dB, Q = 0.7071752369554196; K = tan(pi f0 / rate), Vh = 10^(G / 20), Vb = Vh^0.4996667741545416,
 *             a0 = 1 + K / Q + K^2; b0 = (Vh + Vb K / Q + K^2) / a0, b1 = 2 (K^2 - Vh) / a0, b2 = (Vh - Vb K / Q + K^2) / a0, a1 = 2 (K^2 - 1) / a0,
 *             a2 = (1 - K / Q + K^2) / a0.  High-pass: f0 = 38.13547087602444, Q = 0.5003270373238773, the same K and denominator form;
 *             b = (1, -2, 1), a1 = 2 (K^2 - 1) / a0, a2 = (1 - K / Q + K^2) / a0.  At 48 kHz these are BS.1770-4's printed tables.
 *   filter    per channel on the widened f32 sample, shelf then high-pass, transposed direct form II: y = b0 x + s1; s1 = (b1 x - a1 y) + s2;
 *             s2 = b2 x - a2 y.  The state S = (s1, s2 of the shelf, s1, s2 of the high-pass) is +0.0 when the taps are set and carried across
 *             ticks and runs.
 *   ticks     for tick k of F frames with start state S_k the outputs y[i] are the plain recurrence from S_k, but the next start state is
 *             S_k+1 = Z_k + P S_k: Z_k is the end state of the same walk from the zero state and P = carry[4][4] what the host gets by
 *             walking F zero samples from each unit state (column c: from unit state c).  Row r is evaluated as
 *             ((P[r][0] S0 + P[r][1] S1) + P[r][2] S2) + P[r][3] S3, then Z[r] + that.  This makes the ticks of a run independent of each
 *             other and the records independent of how ticks are grouped into runs; against the uninterrupted recurrence it moves ksq by
 *             rounding only (DESIGN.md section 0.5 has the measured figure).
 *   ksq       per channel 8 f64 partials: partial j adds y[i] * y[i] (the product rounded, then the sum) for i = j (mod 8) in ascending i
 *             from +0.0; then s[j] = s[j] + s[j ^ m] for m = 4, 2, 1; the value is s[0].
 *   windows   momentary_sq of tick t = the sum of (ksq[0] + ksq[1]) over ticks t - momentary_ticks + 1 .. t, added in ascending tick from
 *             +0.0, every tick summed afresh; ticks before the set read +0.0; short_sq the same over short_ticks.  The last 1023 ticks are
 *             carried across runs.  Loudness in LUFS = -0.691 + 10 log10(window sum / (window ticks x frames)).
 *   true peak on the unweighted f32 samples: interp[p-1][j], p = 1 .. 3, j = 0 .. 11, is the f32 nearest to sinc(d) (0.5 + 0.5 cos(pi d / 6)),
 *             d = j - 5 - p / 4, sinc(d) = sin(pi d) / (pi d); v_p[m] = (float) sum over j of (double)interp[p-1][j] * (double)x[m - 11 + j],
 *             accumulated in ascending j in f64 from +0.0; true_peak = the integer maximum of bits & 0x7fffffff over x[m] and v_1..3[m] for
 *             the tick's frames m, read as f32.  Frames before the set read +0.0; the last 11 frames are carried across ticks and runs.
 * A mono port has channels = 1 and every [1] field 0.  A stereo port stored as one float per frame (the fused L == R strip result) gives both
 * channels from that float, equal to MX_FLAG_NO_FUSE's records bit for bit.  Non-finite input propagates (NaN / Inf).
 * Every call to mx_graph_set_loudness resets every tap: filter state, window history and interpolator history go to +0.0 (integration over a
 * programme lives on the host: mx_loudness_gate).  One parameter set holds for every tap of the graph. */
typedef struct { uint32_t momentary_ticks; uint32_t short_ticks; } mx_loudness_params;   /* each 1 .. 1024; 24 and 180 are 400 ms and 3 s at 60 ticks/s */
typedef struct {
    double   ksq[2];        /* K-weighted sum of squares of the tick, per channel */
    double   momentary_sq;  /* window sum over the last momentary_ticks ticks of (ksq[0] + ksq[1]) */
    double   short_sq;      /* the same over short_ticks */
    float    true_peak[2];
    uint32_t frames;
    uint32_t channels;
} mx_loudness_tick;   /* 48 bytes: ksq 0, momentary_sq 16, short_sq 24, true_peak 32, frames 40, channels 44 */
/* Replaces the graph's loudness taps with ports[0..n) (n = 0: none; params may then be NULL and the graph launches nothing for them).
 * Video port: MX_ERR_TYPE.  A node or port out of range, a duplicate (node, port), a port the fusion did not materialise, a window length
 * outside 1 .. 1024, a port whose rate is not above twice the shelf frequency (3 364 Hz): MX_ERR_INVALID.  Waits for outstanding work like a
 * read-back but keeps the automatic second-stream mode on.  Device memory: max_ticks_per_run x n x (48 bytes of records + 64 bytes of walk
 * states) + per tap 64 bytes of filter state, 2 x 1023 doubles of window history, 2 x 22 floats of frame history and 208 bytes of coefficients.
 * mx_graph_adopt_state does not carry taps: set them again on the new graph.  The launches count in the profile calls' ms_total only
 * (MX_PROFILE_KINDS is unchanged).  The per-module path (mx_module_*) exposes no graph handle, so taps cannot be set there. */
int mx_graph_set_loudness(mx_graph* g, const mx_port_ref* ports, size_t n, const mx_loudness_params* params);
/* Ticks [first_tick_in_run, first_tick_in_run + n_ticks) of the last run, laid out [tick][tap] in set order; cap = records dst holds.
 * A window beyond the last run (or a run made before the taps were set), cap < n_ticks x taps, or no taps: MX_ERR_INVALID.  Joins the
 * graph's streams like mx_graph_read_output. */
int mx_graph_read_loudness(mx_graph* g, uint32_t first_tick_in_run, uint32_t n_ticks, mx_loudness_tick* dst, size_t cap);
/* The tables of the spec for one rate and tick length: biquads[10] (shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2), carry[16] (P[r][c] at
 * 4 r + c), interp[36] (interp[p-1][j] at 12 (p - 1) + j); any of them may be NULL.  Host only: touches no device and needs no graph.  A rate
 * that is not finite or not above 3 363.948901911066 (twice the shelf frequency), frames_per_tick outside 1 .. 4 194 304: MX_ERR_INVALID. */
int mx_loudness_tables(double rate, uint32_t frames_per_tick, double* biquads, double* carry, float* interp);
/* Gated integration (BS.1770-4) over n_blocks measurement blocks, in f64 on the host: block i has block_sq[i] (a momentary_sq) over
 * block_frames[i] frames (momentary_ticks x frames) and loudness l_i = -0.691 + 10 log10(block_sq[i] / block_frames[i]).  Keep the blocks with
 * l_i > -70; Gamma = -0.691 + 10 log10(mean of the kept blocks' mean squares) - 10; keep those of them that also have l_i > Gamma;
 * *lufs_integrated = -0.691 + 10 log10 of their mean, or -inf with *blocks_kept = 0 when none is left (blocks_kept may be NULL).  Feed every
 * hop-th tick's momentary_sq: six ticks at 60 ticks/s give the standard's 75 % overlap.  Host only.  A NULL array with n_blocks > 0, a NULL
 * lufs_integrated or a block of 0 frames: MX_ERR_INVALID. */
int mx_loudness_gate(const double* block_sq, const uint32_t* block_frames, size_t n_blocks, double* lufs_integrated, size_t* blocks_kept);

/* Stereo field taps on STEREO output ports of a built graph: per tick the three sums behind the phase-correlation
 * meter, balance and width, with their sums over a window of ticks, and -- with grid != 0 -- a goniometer, the audio counterpart of the
 * vectorscope.  Like a meter, a tap observes a port: no module, no edge, the run order and the fusion plan unchanged; a graph without them
 * launches nothing new.  Meters, spectrum, video scope, loudness and stereo field taps are independent sets and may be set together.  Every run
 * computes the records on the device, once per run after its last span.  BUILD-SPECIFIED (the reference has no such instrument); the numbers
 * are fixed bit for bit (tests/stereo_model.py restates them in numpy); every f64 operation is rounded on its own (no fused multiply-add).
 * A port stored as one float per frame (the fused L == R strip result) reads as L = R = that float, equal to MX_FLAG_NO_FUSE's records bit for
 * bit.  Frames are counted in the port's own rate domain, as for meters.
 *   sum_xy    (xy = ll, rr, lr) the meters' order: 64 partials, partial j adds (double)x[f] * (double)y[f] (exact: 24 + 24 bits) over the
 *             tick's frames f = j (mod 64) in ascending f from +0.0, one f64 rounding per add; then s[j] = s[j] + s[j ^ k] for k = 32, 16, 8,
 *             4, 2, 1; the value is s[0].  sum_ll and sum_rr equal a meter's sum_sq[0] and sum_sq[1] on the same port bit for bit.
 *             Non-finite input propagates into the sums.
 *   win_xy    the sum of sum_xy over ticks t - window_ticks + 1 .. t, added in ascending tick from +0.0, every tick summed afresh (no running
 *             sum: nothing drifts, and the grouping of ticks into runs cannot matter); ticks before the set read +0.0.  The last 1023 ticks
 *             are carried across runs.
 *   nonfinite frames of the tick whose L or R is NaN or +-Inf.
 * Correlation, balance, mid and side energy are NOT in the record: they are quotients and roots of the six sums (mid / side energy =
 * (ll + rr +- 2 lr) / 4); mx_stereo_correlation is the host-side helper for the first.
 *   goniometer  present when grid != 0: a grid x grid table of uint32_t counts, grid 64 or 128.  For every frame with finite L and R:
 *             m = L + R and s = L - R in f32, each rounded once; the cell of a value v is t = floorf(v * z), z = 2^zoom_log2 * grid / 4 (a
 *             power of two: the product is exact), t = fminf(fmaxf(t, -grid / 2), grid / 2 - 1), index (int)t + grid / 2; the frame
 *             increments gon[cell(m)][cell(s)].  zoom_log2 is 0 .. 8; at 0 the grid spans [-2, 2) on both axes.  An m or s that overflows
 *             from finite L, R clamps to the edge like any large value.  A frame with a non-finite L or R is not plotted but counted in
 *             `skipped`.  One counter c per graph: c = 0 and every grid zero when the taps are set; every tick adds its frames to the tap's
 *             grid, then c += 1; when c mod hop == 0 one record per tap is emitted and the grids are cleared.  c and the partly filled grids
 *             are carried across runs.  Counts are integers: the order of accumulation cannot matter.
 *   record    32-byte header uint32_t { tick_in_run (the emitting tick), ticks (= hop), frames (plotted), skipped, grid, zoom_log2,
 *             reserved[2] (0) }, then the table, row-major [cell(m)][cell(s)]: 32 + 4 grid^2 bytes (mx_stereo_gonio_record_bytes).
 * With grid = 0 nothing is allocated or launched for the goniometer and hop is ignored.  One parameter set holds for every tap of the graph.
 * Every call to mx_graph_set_stereo resets every tap and c. */
typedef struct { uint32_t window_ticks /* 1 .. 1024 */, grid /* 0, 64 or 128 */, zoom_log2 /* 0 .. 8 */, hop /* >= 1 when grid != 0 */; } mx_stereo_params;
typedef struct {
    double   sum_ll;        /* this tick */
    double   sum_rr;
    double   sum_lr;
    double   win_ll;        /* the last window_ticks ticks */
    double   win_rr;
    double   win_lr;
    uint32_t frames;
    uint32_t nonfinite;     /* frames of the tick whose L or R is NaN or +-Inf */
} mx_stereo_tick;   /* 56 bytes: sum_ll 0, sum_rr 8, sum_lr 16, win_ll 24, win_rr 32, win_lr 40, frames 48, nonfinite 52 */
/* Replaces the graph's stereo field taps with ports[0..n) (n = 0: none; params may then be NULL and the graph launches nothing for them).
 * Video or mono port: MX_ERR_TYPE.  A node or port out of range, a duplicate (node, port), a port the fusion did not materialise,
 * window_ticks outside 1 .. 1024, a grid other than 0, 64, 128, zoom_log2 > 8, hop = 0 with grid != 0: MX_ERR_INVALID.  Goniometer records
 * of one run (ceil(max_ticks_per_run / hop) x n x record bytes) beyond 4 GiB: MX_ERR_NOMEM (raise hop).  Waits for outstanding work like a
 * read-back but keeps the automatic second-stream mode on.  Device memory: max_ticks_per_run x n x 56 bytes of records, per tap 2 x 1023 x 3
 * doubles of window history, and with a goniometer one record per tap of carried grid plus the run's records.  mx_graph_adopt_state does not
 * carry taps: set them again on the new graph.  The launches count in the profile calls' ms_total only (MX_PROFILE_KINDS is unchanged). */
int mx_graph_set_stereo(mx_graph* g, const mx_port_ref* ports, size_t n, const mx_stereo_params* params);
/* Ticks [first_tick_in_run, first_tick_in_run + n_ticks) of the last run, laid out [tick][tap] in set order; cap = records dst holds.
 * A window beyond the last run (or a run made before the taps were set), cap < n_ticks x taps, or no taps: MX_ERR_INVALID.  Joins the
 * graph's streams like mx_graph_read_output. */
int mx_graph_read_stereo(mx_graph* g, uint32_t first_tick_in_run, uint32_t n_ticks, mx_stereo_tick* dst, size_t cap);
/* The goniometer records the last run emitted, [emission][tap in set order], mx_stereo_gonio_record_bytes each; *n_records = emissions x taps
 * (0 when the run emitted none; n_records may be NULL).  No taps, taps set with grid = 0, no run since the taps were set, or cap_bytes too
 * small: MX_ERR_INVALID.  Joins the graph's streams like mx_graph_read_output. */
int mx_graph_read_goniometers(mx_graph* g, void* dst, size_t cap_bytes, uint32_t* n_records);
/* Bytes of one goniometer record: 32 + 4 grid^2 (32 with grid = 0).  Host only.  A grid other than 0, 64, 128 or a NULL argument: MX_ERR_INVALID. */
int mx_stereo_gonio_record_bytes(const mx_stereo_params* params, size_t* bytes);
/* *r = lr / sqrt(ll * rr) in f64, clamped to [-1, 1]; 0.0 when ll * rr is not a positive finite number (silence on one side reads 0, not NaN)
 * or the quotient is NaN.  Feed a record's sums or its window sums.  Host only: touches no device and needs no graph.  NULL r: MX_ERR_INVALID. */
int mx_stereo_correlation(double ll, double rr, double lr, double* r);

/* Look-ahead limiter taps on audio output ports of a built graph: the one tap set that acts on level.  A tap
 * observes a port like a meter -- no module, no edge, the run order, the fusion plan and the port itself unchanged; a graph without them
 * launches nothing new -- and writes a LIMITED COPY of the port, delayed by the lookahead, plus one small record per tick.  The six tap sets
 * are independent and may be set together.  Every run computes copies and records on the device, once per run after its last span.
 * BUILD-SPECIFIED (the reference has no limiter; its OutputDevice reports clip and its sinks clamp); the numbers are fixed bit for bit
 * (tests/limiter_model.py restates them in numpy).  The arithmetic is feed-forward -- a sliding minimum, then FIR smoothing of the gain -- so
 * every output sample is a function of a bounded window of input frames, and the copies are bit-identical however ticks are grouped into runs.
 *   parameters  ceiling c: finite, 2^-20 <= c <= 1; lookahead D in frames of the port's own rate domain, 0 <= D <= 512.  One set per graph.
 *   stream    a tap treats its port as one stream of frames n = 0, 1, ... that starts when the taps are set and continues across ticks and
 *             runs (first_tick may jump: the stream does not care).  Frames before n = 0 are +0.0.  Every f32 operation is rounded on its
 *             own (no fused multiply-add).
 *   level     a[n] = the f32 whose bits are max(bits(L) & 0x7fffffff, bits(R) & 0x7fffffff): the channels of a stereo port are linked; a
 *             mono port has one.  A stereo port stored as one float per frame (the fused L == R strip result) reads as L = R = that float,
 *             equal to MX_FLAG_NO_FUSE's copy and records bit for bit.
 *   required  r[n] = +0.0 if bits(a) >= 0x7f800000 (Inf, NaN); 1.0 if a <= c; else c / min(a, 65536.0f), the correctly rounded f32 quotient
 *             (the cap keeps every quotient normal; louder samples meet the final clamp).
 *   hold      m[n] = min(r[n - D] .. r[n]).
 *   smoothing s[n]: acc = +0.0; for k = 0 .. D ascending: p = w[k] * m[n - k]; acc = acc + p.  w[k] = the f32 nearest to h[k] / sum h,
 *             h[k] = 1 - cos(2 pi (k + 1) / (D + 2)); D = 0: w = {1}.  mx_limiter_weights returns the very table the kernel uses.
 *   gain      q = min(m[n], m[n - D]); g[n] = 1.0 if q == 1.0, else min(s[n], r[n - D]).  The first branch makes the limiter exactly
 *             transparent where nothing within 2 D frames needs limiting; the min makes the ceiling a guarantee whatever the weights round to.
 *   output    per channel x = input[n - D]; a non-finite x gives +0.0 and is counted; else y[n] = max(-c, min(c, x * g[n])).  The limited copy
 *             is the port delayed by D frames in the port's LOGICAL layout: interleaved stereo also for a port stored as one float per frame.
 *   record    over the frames n of the tick: min_gain the smallest g (integer minimum of its bits), peak_out the largest bits of |y| read as
 *             f32, limited the frames with g < 1, nonfinite the samples replaced, frames and channels of the port.
 * Carried per tap: the last 2 D input frames, handed from run to run (a run shorter than 2 D frames shifts them).  Every call to
 * mx_graph_set_limiters resets every tap: the stream starts again from silence.  mx_graph_adopt_state carries no taps. */
typedef struct { float ceiling; uint32_t lookahead; } mx_limiter_params;
#define MX_LIMITER_MAX_LOOKAHEAD 512u
typedef struct {
    float    min_gain;      /* smallest gain of the tick; 1.0 when nothing was limited */
    float    peak_out;      /* largest |y| of the tick: <= ceiling */
    uint32_t limited;       /* frames with gain < 1 */
    uint32_t nonfinite;     /* samples (not frames) replaced by +0.0 */
    uint32_t frames;
    uint32_t channels;
} mx_limiter_tick;   /* 24 bytes: min_gain 0, peak_out 4, limited 8, nonfinite 12, frames 16, channels 20 */
/* Replaces the graph's limiter taps with ports[0..n) (n = 0: none; params may then be NULL and the graph launches nothing for them).
 * Video port: MX_ERR_TYPE.  A node or port out of range, a duplicate (node, port), a port the fusion did not materialise, a ceiling that is
 * not finite or outside [2^-20, 1], a lookahead above 512: MX_ERR_INVALID.  Device memory that cannot be had: MX_ERR_NOMEM, and the graph is
 * left without limiter taps.  Waits for outstanding work like a read-back but keeps the automatic second-stream mode on.  Device memory:
 * max_ticks_per_run x (the sum over the taps of frames x channels floats + n x 24 bytes of records), per tap 2 x 2 x 1024 floats of history,
 * and the weights.  The launches count in the profile calls' ms_total only (MX_PROFILE_KINDS is unchanged). */
int mx_graph_set_limiters(mx_graph* g, const mx_port_ref* ports, size_t n, const mx_limiter_params* params);
/* Ticks [first_tick_in_run, first_tick_in_run + n_ticks) of the last run, laid out [tick][tap] in set order; cap = records dst holds.
 * A window beyond the last run (or a run made before the taps were set), cap < n_ticks x taps, or no taps: MX_ERR_INVALID.  Joins the
 * graph's streams like mx_graph_read_output. */
int mx_graph_read_limiters(mx_graph* g, uint32_t first_tick_in_run, uint32_t n_ticks, mx_limiter_tick* dst, size_t cap);
/* The limited copy of tap `tap` (its index in set order) over the same kind of window: n_ticks x frames x channels floats, ticks back to
 * back; *n_samples = that count (n_samples may be NULL; samples = NULL with cap = 0 asks for the count alone).  A tap out of range, a window
 * beyond the last run, cap too small: MX_ERR_INVALID.  _i16 gives the same samples in the sinks' format (mx_graph_read_output_i16: clamp to
 * [-1, 1], x 32767, truncation); since |y| <= ceiling <= 1 the clamp never acts. */
int mx_graph_read_limited(mx_graph* g, size_t tap, uint32_t first_tick_in_run, uint32_t n_ticks, float* samples, size_t cap, size_t* n_samples);
int mx_graph_read_limited_i16(mx_graph* g, size_t tap, uint32_t first_tick_in_run, uint32_t n_ticks, int16_t* samples, size_t cap, size_t* n_samples);
/* For zero-copy consumers: *dev = tap `tap`'s copy of tick 0 of a run on the device; tick t of the run starts *floats_per_tick floats
 * further per tick (the copies of all taps of one tick lie together) and holds frames x channels floats.  The call orders the graph's
 * stream behind the last run's limiter launches (also those that went out behind a Mixer bank on the second stream); call it again, or
 * mx_graph_sync, after a later run before reading on another stream.  The pointer holds until the taps are set again or the graph grows. */
int mx_graph_limited_device_ptr(mx_graph* g, size_t tap, void** dev, size_t* floats_per_tick);
/* The smoothing weights of the spec for one lookahead: w[lookahead + 1].  Host only: touches no device and needs no graph.  A lookahead above
 * 512 or a NULL w: MX_ERR_INVALID. */
int mx_limiter_weights(uint32_t lookahead, float* w);

/* Tempo taps on audio output ports of a built graph: the autocorrelation of an onset function per port, from which a
 * host reads the tempo (BPM) a DJ beat-matches by.  Like a meter, a tap observes a port: no module, no edge, the run order and the fusion plan
 * unchanged; a graph without them launches nothing new.  The seven tap sets are independent and may be set together.  Every run computes the
 * records on the device, once per run after its last span.  BUILD-SPECIFIED (the reference has no such instrument); everything below the
 * mid signal is integer arithmetic, so the records are fixed count for count (tests/tempo_model.py restates them in numpy and Python
 * integers), they are identical however ticks are grouped into runs, and the order of accumulation cannot matter.
 *   parameters  hop_frames H: 64, 128 or 256; window_hops W: 64 .. 4096; max_lag L: 16 .. 1024 and L <= W; emit_ticks >= 1.  One set per graph.
 *   stream    a tap treats its port as one stream of frames that starts when the taps are set (frame 0) and continues across ticks and
 *             runs, in the port's own rate domain (first_tick may jump: the stream does not care).  A mono port, and a stereo port stored as
 *             one float per frame (the fused L == R strip result), read as L = R = x: equal to MX_FLAG_NO_FUSE's records byte for byte.
 *   mid       m = L + R in f32, rounded once.
 *   quantise  a non-finite m (NaN, +-Inf, also from finite L and R) gives q = 0 and is counted in `nonfinite`; else
 *             q = (uint32_t)(fminf(fabsf(m), 4.0f) * 1048576.0f): the product is exact, the conversion truncates, q <= 2^22.
 *   energy    hop h is the stream's frames [h H, (h + 1) H): E[h] = the sum of q^2 as uint64_t, at most 2^52.
 *   amplitude A[h] = floor(sqrt(E[h])), the exact integer root; A[-1] = 0.
 *   onset     o[h] = max(A[h] - A[h - 1], 0) >> 6, at most 2^20; o of a negative hop is 0.
 *   emission  one counter c per graph: c = 0 when the taps are set; every tick does c += 1, and when c mod emit_ticks == 0 every tap emits a
 *             record.  hl is the last hop whose final frame lies in this tick or an earlier one (none: the whole table is zero).  For
 *             l = 0 .. L - 1: R[l] = the sum over j = 0 .. W - 1 of o[hl - j] * o[hl - j - l] as uint64_t (at most 2^52: no overflow).  Every
 *             record is summed afresh from the carried history of W + L - 1 onsets: there is no running sum.
 *   record    32-byte header uint32_t { tick_in_run (the emitting tick), hops_complete (hl + 1, saturating), nonfinite (frames since the
 *             previous emission), hop_frames, window_hops, max_lag, reserved[2] (0) }, then R[0 .. L) as uint64_t: 32 + 8 L bytes
 *             (mx_tempo_record_bytes).
 * Carried across runs per tap: the energy of the hop in progress, A of the last complete hop, the onset history and nonfinite; per graph: c.
 * Every call to mx_graph_set_tempo resets every tap and c.  mx_graph_adopt_state carries no taps. */
typedef struct { uint32_t hop_frames /* 64, 128 or 256 */, window_hops /* 64 .. 4096 */, max_lag /* 16 .. 1024, <= window_hops */, emit_ticks /* >= 1 */; } mx_tempo_params;
/* Replaces the graph's tempo taps with ports[0..n) (n = 0: none; params may then be NULL and the graph launches nothing for them).  Video port:
 * MX_ERR_TYPE.  A node or port out of range, a duplicate (node, port), a port the fusion did not materialise, a parameter outside its range:
 * MX_ERR_INVALID.  The records of one run (ceil(max_ticks_per_run / emit_ticks) x n x record bytes) beyond 4 GiB: MX_ERR_NOMEM (raise
 * emit_ticks).  Device memory that cannot be had: MX_ERR_NOMEM, and the graph is left without tempo taps.  Waits for outstanding work like a
 * read-back but keeps the automatic second-stream mode on.  Device memory: the run's records, and per tap 2 x (W + L - 1 + the hops of the
 * longest run) onsets of 4 bytes plus 8 bytes per hop of the longest run.  The launches count in the profile calls' ms_total only
 * (MX_PROFILE_KINDS is unchanged). */
int mx_graph_set_tempo(mx_graph* g, const mx_port_ref* ports, size_t n, const mx_tempo_params* params);
/* The records the last run emitted, [emission][tap in set order], mx_tempo_record_bytes each; *n_records = emissions x taps (0 when the run
 * emitted none; n_records may be NULL).  No taps, no run since the taps were set, or cap_bytes too small: MX_ERR_INVALID.  Joins the graph's
 * streams like mx_graph_read_output. */
int mx_graph_read_tempo(mx_graph* g, void* dst, size_t cap_bytes, uint32_t* n_records);
/* Bytes of one tempo record: 32 + 8 max_lag.  Host only.  A parameter outside its range or a NULL argument: MX_ERR_INVALID. */
int mx_tempo_record_bytes(const mx_tempo_params* params, size_t* bytes);
/* Tempo of one record, in f64 on the host (needs no graph): the candidate lags are the integers in
 * [60 rate / (H bpm_hi), 60 rate / (H bpm_lo)] intersected with [1, L - 2]; l* is the first maximum of R over them;
 * d = 0.5 (R[l* - 1] - R[l* + 1]) / (R[l* - 1] - 2 R[l*] + R[l* + 1]) when that denominator is negative, else 0 (parabolic refinement);
 * *bpm = 60 rate / (H (l* + d)), *confidence = R[l*] / R[0].  R[0] == 0 (silence, or nothing but non-finite frames) or no candidate lag:
 * *bpm = 0, *confidence = 0.  rate: the port's own frames per second.  A NULL argument, a header whose parameters are outside their ranges, a
 * rate or bound that is not finite and positive, or bpm_hi < bpm_lo: MX_ERR_INVALID. */
int mx_tempo_bpm(const void* record, double rate, double bpm_lo, double bpm_hi, double* bpm, double* confidence);

/* Tonality taps on audio output ports of a built graph: a constant-Q analysis of a decimated stream per port, from
 * which a host reads the pitch-class profile and the musical key a DJ mixes harmonically by.  ("key" and "chroma" name the video keyer
 * here, so this set is called tonality.)  Like a meter, a tap observes a port: no module, no edge, the run order and the fusion plan unchanged;
 * a graph without them launches nothing new.  The audio tap sets are independent and may be set together.  Every run computes the records on
 * the device, once per run after its last span.  BUILD-SPECIFIED (the reference has no such instrument); everything after the mid signal is
 * integer arithmetic, so the records are fixed count for count (tests/tonality_model.py restates them in numpy and Python integers), they
 * are identical however ticks are grouped into runs, and the order of accumulation cannot matter.
 *   parameters  decim D: 4 or 8; hop_frames Hc (decimated frames): 128, 256 or 512; octaves O: 2 .. 6, B = 12 O bins; f_lo_mhz >= 1, the lowest
 *             bin's frequency in millihertz (65406 = C2); emit_ticks >= 1.  One set per graph.
 *   stream    a tap treats its port as one stream of frames that starts when the taps are set (frame 0) and continues across ticks and
 *             runs, in the port's own rate domain (first_tick may jump: the stream does not care).  A mono port, and a stereo port stored as
 *             one float per frame (the fused L == R strip result), read as L = R = x: equal to MX_FLAG_NO_FUSE's records byte for byte.
 *   mid       m = L + R in f32, rounded once.
 *   quantise  a non-finite m (NaN, +-Inf, also from finite L and R) gives q = 0 and is counted in `nonfinite`; else
 *             q = (int32_t)(fminf(fmaxf(m, -2.0f), 2.0f) * 8192.0f): the product is exact, the conversion truncates, |q| <= 2^14.
 *   decimate  fs_d = rate / D, Tf = 8 D taps: d[n] = (sum over k < Tf of c[k] * q[n D - k]) >> 15, an arithmetic shift (floor); q at a
 *             negative index is 0; d[n] is complete in the tick that holds input frame n D.  c[k] = round(2^15 h[k] / sum h), where
 *             h[k] = sin(2 pi (0.45 / D) t) / (pi t) * (0.5 - 0.5 cos(2 pi (k + 1) / (Tf + 1))), t = k - (Tf - 1) / 2: a Hann-windowed sinc
 *             with cutoff 0.45 fs_d, centred at (Tf - 1) / 2, in f64 on the host.  sum |c[k]| <= 65534, so |d| < 32767: d fits an int16_t
 *             and nothing is clamped.
 *   kernels   Q = 17; f_b = f_lo * 2^(b / 12) for b < B; N_b = ceil(Q * fs_d / f_b).  N_0 > 2048, or f_{B-1} * 2^(1/24) >= 0.45 fs_d:
 *             MX_ERR_INVALID.  For n < N_b: w_b[n] = 0.5 - 0.5 cos(2 pi (n + 1) / (N_b + 1)), phi = 2 pi f_b (n - (N_b - 1)) / fs_d,
 *             K_re[b][n] = round(16384 w_b[n] cos(phi)), K_im[b][n] = round(-16384 w_b[n] sin(phi)), in f64 on the host; n = N_b - 1 is
 *             the newest frame.  mx_tonality_tables returns c, N_b and K as the device uses them.
 *   hop       hop h ends at decimated frame e_h = (h + 1) Hc - 1 and is complete in the tick that holds input frame e_h * D.
 *             S_re = sum over n < N_b of K_re[b][n] * d[e_h - (N_b - 1) + n], likewise S_im; d at a negative index is 0; |S| <= 2^40.
 *             M_b[h] = floor(sqrt((S_re >> 10)^2 + (S_im >> 10)^2)): the shifts are floor, the sum is below 2^61, the root is the exact
 *             integer root.
 *   emission  one counter c per graph: c = 0 when the taps are set; every tick does c += 1, and when c mod emit_ticks == 0 every tap emits a
 *             record: C[b] = the sum of M_b[h] over the hops completed since the previous emission, as uint64_t.  Nothing is windowed:
 *             the host sums records for a longer view (mx_tonality_chroma).
 *   record    32-byte header uint32_t { tick_in_run (the emitting tick), hops (completed since the previous emission), nonfinite (frames
 *             arrived since the previous emission), decim, hop_frames, octaves, f_lo_mhz, 0 }, then C[0 .. B) as uint64_t: 32 + 8 B bytes
 *             (mx_tonality_record_bytes).
 * Carried across runs per tap: the Tf - 1 + (D - 1) newest quantised frames, the newest 2047 + Hc - 1 decimated frames, C[b] and hops so
 * far, and nonfinite; per graph: c.  Every call to mx_graph_set_tonality resets every tap and c.  mx_graph_adopt_state carries no taps. */
typedef struct { uint32_t decim /* D: 4 or 8 */, hop_frames /* Hc, in decimated frames: 128, 256 or 512 */, octaves /* O: 2 .. 6; B = 12 O bins */, f_lo_mhz /* lowest bin's frequency in millihertz, e.g. 65406 = C2 */, emit_ticks /* >= 1 */; } mx_tonality_params;
/* Replaces the graph's tonality taps with ports[0..n) (n = 0: none; params may then be NULL and the graph launches nothing for them).  Video
 * port: MX_ERR_TYPE.  A node or port out of range, a duplicate (node, port), a port the fusion did not materialise, a parameter outside its
 * range, kernels that do not exist at a port's own rate (N_0 > 2048, or the top bin at 0.45 fs_d): MX_ERR_INVALID.  The records of one run
 * (ceil(max_ticks_per_run / emit_ticks) x n x record bytes) beyond 4 GiB: MX_ERR_NOMEM (raise emit_ticks).  Device memory that cannot be
 * had: MX_ERR_NOMEM, and the graph is left without tonality taps.  Waits for outstanding work like a read-back but keeps the automatic
 * second-stream mode on.  Device memory: the run's records, one table set per rate domain among the taps, and per tap 2 x (2047 + Hc - 1 +
 * the decimated frames of the longest run) x 2 bytes.  The launches count in the profile calls' ms_total only (MX_PROFILE_KINDS is unchanged). */
int mx_graph_set_tonality(mx_graph* g, const mx_port_ref* ports, size_t n, const mx_tonality_params* params);
/* The records the last run emitted, [emission][tap in set order], mx_tonality_record_bytes each; *n_records = emissions x taps (0 when the
 * run emitted none; n_records may be NULL).  No taps, no run since the taps were set, or cap_bytes too small: MX_ERR_INVALID.  Joins the
 * graph's streams like mx_graph_read_output. */
int mx_graph_read_tonality(mx_graph* g, void* dst, size_t cap_bytes, uint32_t* n_records);
/* Bytes of one tonality record: 32 + 8 x 12 x octaves.  Host only.  A parameter outside its range or a NULL argument: MX_ERR_INVALID. */
int mx_tonality_record_bytes(const mx_tonality_params* params, size_t* bytes);            /* 32 + 8 B */
/* The tables of the spec for a port of `rate` frames per second, as the device uses them (host only, f64): fir[8 D] = c, len[B] = N_b, and
 * kern[sum(len)][2] = { K_re, K_im }, bin after bin (kern NULL: sizes only); *kern_pairs = sum(len) (may be NULL).  A NULL params, fir or
 * len, a parameter outside its range, a rate that is not finite and positive, N_0 > 2048 or the top bin at 0.45 fs_d: MX_ERR_INVALID. */
int mx_tonality_tables(double rate, const mx_tonality_params* params, int16_t* fir /* 8 D */, uint32_t* len /* B */,
                       int16_t* kern /* sum(len) x {re, im}, bin after bin; NULL: sizes only */, size_t* kern_pairs);
/* Pitch-class profile of n_records >= 1 back-to-back records of one tap, in f64 on the host (needs no graph): C[b] summed over the records
 * as integers, divided by N_b (recomputed from the header and rate), each bin folded into pitch class
 * (round(12 log2(f_lo / 16.351597831)) + b) mod 12 with C = 0, and the twelve scaled to sum 1; all zero stays zero.  Records whose headers
 * (decim, hop_frames, octaves, f_lo_mhz) disagree or are outside their ranges, kernels that do not exist at `rate`, a NULL argument or
 * n_records = 0: MX_ERR_INVALID. */
int mx_tonality_chroma(const void* records, size_t n_records, double rate, double chroma[12]);   /* host, f64 */
/* Key of a pitch-class profile, in f64 on the host: the Pearson correlation r of chroma with the 24 rotations of the Krumhansl-Kessler
 * profiles (major 6.35 2.23 3.48 2.33 4.38 4.09 2.52 5.19 2.39 3.66 2.29 2.88; minor 6.33 2.68 3.52 5.38 2.60 3.53 2.54 4.75 3.98 2.69 3.34
 * 3.17).  *key = 0 .. 11: major on that tonic (C = 0); 12 .. 23: minor on tonic key - 12; the first maximum wins; *confidence = the best r
 * minus the second best.  A chroma whose entries are all equal (all zero included): *key = -1, *confidence = 0.  A NULL argument or a chroma entry
 * that is not finite: MX_ERR_INVALID. */
int mx_tonality_key(const double chroma[12], int* key, double* confidence);                     /* host, f64 */

/* Plotter indication (src/module/plotter.rs:37-56) for tick `tick_in_run` of the last run:
 * *fired = 1 and SPT floats in each of left/right when it fired (every 6th call, input connected). */
int mx_graph_read_plotter(mx_graph* g, uint32_t node, uint32_t tick_in_run, float* left, float* right, int* fired);

/* Per-kind device time of the last profiled run (the PerformanceInfo analogue,
 * src/engine/timing.rs:86-94): run once with hipEvents around every launch group. */
int mx_graph_profile_run(mx_graph* g, uint64_t first_tick, uint32_t n_ticks, float* ms_by_kind /* MX_PROFILE_KINDS */, float* ms_total);
/* Same, accumulated over many asynchronous runs: while enabled every mx_graph_run_ticks records a
 * hipEvent before/after each launch group on the graph's stream (no synchronisation);
 * collect synchronises and returns the sums (ms) and the number of runs they cover. */
int mx_graph_profile_enable(mx_graph* g, int on);
int mx_graph_profile_collect(mx_graph* g, float* ms_by_kind /* MX_PROFILE_KINDS */, float* ms_total, uint32_t* n_runs);

/* The reference's performance panel (PerformanceInfo, protocol/src/lib.rs:32-59, filled by EngineStat::report,
 * src/engine/timing.rs:46-60) from the most recent profiled run (mx_graph_profile_run, or profile_enable + collect):
 *   realtime       the tick finished inside its budget (timing.rs:33)
 *   lag            0 none, 1 Recent (< 5 s ago), 2 Active (< 100 ms ago): a tick ran over its budget (util.rs:47-60)
 *   tick_budget_us 1e6 / ticks_per_second (timing.rs:9)
 *   module_us[i]   PerformanceAccount::Module(i), "last" metric, per tick: the time of the launch that served the module,
 *                  split evenly over the modules (and folded modules) that launch served
 *   engine_us      PerformanceAccount::Engine = tick time - sum of module accounts (timing.rs:43) */
typedef struct mx_performance_info {
    int32_t realtime; int32_t lag; uint32_t tick_rate; uint32_t n_modules;
    uint64_t tick_budget_us; uint64_t engine_us;
} mx_performance_info;
int mx_graph_performance_info(mx_graph* g, mx_performance_info* info, uint64_t* module_us /* [cap >= n nodes] or NULL */, size_t cap);

/* Topology edit (Engine::client_update, src/engine.rs:277-398): modules persist while connections are added and removed.
 * Build the edited graph with mx_graph_build, then let it take over the state of every module that survives:
 * old_node_of_new[i] = index in `old_graph` of the module that is node i of `new_graph`, or -1 for a new module
 * (EqThree poles and delay line, Envelope state, FIR / resampler history, Plotter count, VideoMixer stored frames and
 * scalers, pending video sources).  Kinds must match (MX_ERR_TYPE).  VideoMixers are MOVED: destroy `old_graph`
 * afterwards, do not run it.  A FIR / resampler whose length changed starts from silence.  A module that a graph never runs
 * (it sits in a cycle that feeds no terminal module, src/engine.rs:428-430) persists like any other: its state waits, from
 * edit to edit, until a graph runs it again. */
int mx_graph_adopt_state(mx_graph* new_graph, mx_graph* old_graph, const int32_t* old_node_of_new, size_t n);

/* Ingest re-blocking (StreamInput::run_tick, src/module/stream_input.rs:92-124): decoded audio arrives as i16 frames of
 * any length; every tick takes exactly 2 * SPT interleaved samples from the queue, a partly consumed frame stays queued,
 * and what the queue cannot fill is zeroed.  mx_pcm_ring_feed re-blocks n_ticks ticks into a SOURCE_STEREO node
 * (H2D as i16, sample / 32768 on the device, stream_input.rs:167-173); *zero_filled = samples it had to zero. */
typedef struct mx_pcm_ring mx_pcm_ring;
int mx_pcm_ring_create(mx_pcm_ring** out);
void mx_pcm_ring_destroy(mx_pcm_ring* r);
int mx_pcm_ring_push_i16(mx_pcm_ring* r, const int16_t* samples, size_t n_samples);
int mx_pcm_ring_queued(const mx_pcm_ring* r, size_t* n_samples);
int mx_pcm_ring_feed(mx_pcm_ring* r, mx_graph* g, uint32_t node, uint32_t n_ticks, size_t* zero_filled);

/* ---- the deck: a track in device memory played at variable speed into a SOURCE_STEREO node ----
 * BUILD-SPECIFIED (no reference module): the pitch fader, cue jump, loop roll, brake and back-spin a host would otherwise resample on the CPU and push over PCIe
 * every tick.  A deck is a feeder of a MX_KIND_SOURCE_STEREO node, in the family of mx_pcm_ring_feed: an object of its own that owns a device-resident track and,
 * before a run, writes that run's ticks into the node's port buffer with ONE kernel launch for all decks and ticks of the call.  The graph itself is unchanged.
 *
 * TRACK     stereo i16 interleaved (4 bytes per frame), n_frames frames, 1 <= n_frames <= 2^30, zeroed at creation.  Frames outside [0, n_frames) read as +0.  A sample
 *           is (float)s / 32768.0f (stream_input.rs:167-173; exact).
 * POSITION  pos: int64 in Q32.32 track frames.  step: the advance per output frame, 2^32 = unity, negative = backwards, |step| <= 4 * 2^32.  A tick of spt output
 *           frames has (pos, step, dstep); frame n of it reads the track at
 *               u(n) = pos + n * step + dstep * (n * (n - 1) / 2)
 *           and after the tick pos = u(spt), step += spt * dstep.  64-bit integer arithmetic throughout: exact, and independent of how ticks are grouped into feeds.
 * PARAMS    mx_deck_params: step_q32 the TARGET step; slew_q32 the largest change of step per output frame, 0 .. 2^24 (0: the step jumps); loop_in < loop_out in
 *           frames; flags MX_DECK_PLAY | MX_DECK_LOOP.  With MX_DECK_LOOP: 0 <= loop_in < loop_out <= n_frames; without it the loop points are not looked at.
 * A TICK    begins with these steps, in this order:
 *             1. a pending seek sets pos;  2. pending parameters replace the current ones;
 *             3. pos is clamped to [-2^20, n_frames + 2^20] frames (a deck left running past its end cannot overflow);
 *             4. the tick is LOOPING when MX_DECK_LOOP is set and either the previous tick was looping under the same (loop_in, loop_out), or
 *                loop_in * 2^32 <= pos < loop_out * 2^32;
 *             5. without MX_DECK_PLAY the tick is written as zeros, pos and step stand still, and its record has dstep = 0, bank = 0.  Otherwise the slew is resolved:
 *                slew = 0: step = target, dstep = 0.  Else dstep = clamp((target - step) / spt, -slew, +slew) with C's truncating division, and if that is 0,
 *                step = target.  (A brake, a spin-up, a pitch bend without a click.)
 *           In a looping tick every u(n), and pos after the tick, is folded: u' = in_q + floormod(u - in_q, len_q), in_q = loop_in * 2^32, len_q = (loop_out - loop_in) * 2^32
 *           (floormod: the remainder with the sign of len_q, i.e. in [0, len_q)); in both directions and for any number of wraps per tick.  In any other tick u' = u.
 *           It follows that a loop set with the head inside it always catches (how loop buttons work), that a loop shorter than one tick's travel may be passed over when
 *           it is entered from outside, and that a seek while the loop stays set lands folded into the loop (clear MX_DECK_LOOP in the same event to leave it).
 *           The taps around a folded position read the track's LINEAR neighbours; they are not folded.
 * FILTER    windowed-sinc polyphase, L = 32 taps, P = 256 phases, blended linearly between neighbouring phase rows; four banks b with cutoff fc_b = 1, 3/4, 1/2, 1/4
 *           of the output Nyquist.  With idx = u' >> 32 (arithmetic), p = (u' >> 24) & 255, w = (double)(u' & 0xFFFFFF) * 2^-24, per channel, acc = 0.0, for k = 0 .. 31
 *           ascending:
 *               c_k = (double)T[b][p][k] + w * ((double)T[b][p + 1][k] - (double)T[b][p][k]);      acc = acc + c_k * (double)x[idx - 15 + k];
 *           every multiply and add a separate f64 operation (never fused), acc rounded once to f32.  MX_FLAG_FP_CONTRACT does not apply: a deck is no graph member.
 *           The bank is chosen per tick from m = max(|step|, |step + (spt - 1) * dstep|) (step as resolved in 5.) by integer comparison:
 *               m <= 2^32: 0;   else 3 m <= 4 * 2^32: 1;   else m <= 2 * 2^32: 2;   else 3.
 * TABLES    T[b]: P + 1 = 257 rows of L = 32 f32.  T[b][p][k] = g(fc_b, (k - 15) - p / 256) / (the sum of g over the row's 32 k), rounded to the nearest f32, where
 *               g(fc, x) = fc * sinc(fc * x) * I0(9 * sqrt(1 - (x / 16)^2)) / I0(9),   sinc(t) = sin(pi t) / (pi t), sinc(0) = 1,   I0 the modified Bessel function
 *           (|x| <= 16 for every entry).  DC passes at gain 1.  In bank 0, rows 0 and 256 are exact unit impulses at k = 15 and k = 16, so AT step = 2^32 FROM AN
 *           INTEGER POSITION THE OUTPUT IS THE TRACK, BIT FOR BIT.
 * RECORDS   mx_deck_tick, one per tick of the last feed: pos / step as the tick began (after 1. - 5.), dstep, loop_in and loop_len in frames (0, 0 unless looping),
 *           bank, and flags: MX_DECK_TICK_PLAY, MX_DECK_TICK_LOOPING, and for a playing tick that is not looping, with m as above,
 *               MX_DECK_TICK_BEFORE  when pos + (spt - 1) * m <  -16 * 2^32             (no tap of the tick reaches frame 0: the tick is zeros),
 *               MX_DECK_TICK_PAST    when pos - (spt - 1) * m >= (n_frames + 15) * 2^32 (no tap reaches below n_frames: zeros).
 * Key-lock (a change of tempo without a change of pitch) is an optional way to render a playing tick: see KEY-LOCK below the deck's calls.
 * Out of scope: more than two channels, tracks above 2^30 frames, a deck as a member of the graph.
 */
#define MX_DECK_PLAY 1u
#define MX_DECK_LOOP 2u
#define MX_DECK_TICK_PLAY 1u
#define MX_DECK_TICK_LOOPING 2u
#define MX_DECK_TICK_BEFORE 4u
#define MX_DECK_TICK_PAST 8u
#define MX_DECK_TAPS 32
#define MX_DECK_PHASES 256
#define MX_DECK_BANKS 4
#define MX_DECK_CHUNK 256        /* output frames one workgroup of the feed kernel writes (a lane per frame); tests size their tick lengths around it */
#define MX_DECK_MAX_SPT 1048576  /* frames per tick mx_deck_plan / mx_deck_feed accept */
typedef struct mx_deck mx_deck;
typedef struct { int64_t step_q32; int64_t slew_q32; int64_t loop_in; int64_t loop_out; uint32_t flags; uint32_t _pad; } mx_deck_params;
/* where the head stands between ticks: pos, the CURRENT step, the current parameters, and whether the last tick was looping, under which points */
typedef struct { int64_t pos_q32; int64_t step_q32; mx_deck_params params; int64_t last_loop_in; int64_t last_loop_out; uint32_t last_looping; uint32_t _pad; } mx_deck_head;
typedef struct { int64_t pos_q32; int64_t step_q32; int64_t dstep_q32; int64_t loop_in; int64_t loop_len; uint32_t flags; uint32_t bank; } mx_deck_tick;

/* A zeroed track of n_frames on `device` (-1: the current one).  The head starts at pos 0, step 0, params all 0 (not playing).  n_frames outside 1 .. 2^30: MX_ERR_INVALID. */
int mx_deck_create(uint64_t n_frames, int device, mx_deck** out);
void mx_deck_destroy(mx_deck* d);
/* Fill frames [first_frame, first_frame + n_frames) from `interleaved` (L R L R ..., 2 x n_frames int16).  Synchronous: the host buffer is the caller's again on return,
 * so a long track can be loaded in pieces while the head plays elsewhere (a piece a feed in flight is reading is the caller's race).  A feed waits for the last load
 * issued before it.  A range outside the track: MX_ERR_INVALID. */
int mx_deck_load_i16(mx_deck* d, uint64_t first_frame, const int16_t* interleaved, uint64_t n_frames);
/* Parameters / a seek (Q32.32 frames, any value: step 3 clamps it) that take effect at tick 0 of the NEXT feed: mx_deck_schedule(d, 0, params, NULL) and (d, 0, NULL, &pos). */
int mx_deck_set(mx_deck* d, const mx_deck_params* params);
int mx_deck_seek(mx_deck* d, int64_t pos_q32);
/* ... at tick `tick_in_feed` of the next feed (a 2048-tick submission is 34 s of music).  Either may be NULL.  A later params / seek for the same tick replaces an
 * earlier one; at one tick the seek applies before the params (steps 1., 2.).  Params are checked here (mx_deck_check).  The feed clears the schedule; a feed that does not
 * reach a scheduled tick fails with MX_ERR_INVALID and drops the schedule, like mx_graph_run_ticks. */
int mx_deck_schedule(mx_deck* d, uint32_t tick_in_feed, const mx_deck_params* params, const int64_t* seek_pos_q32);
/* Host only: the parameter rules alone (MX_OK or MX_ERR_INVALID, mx_last_error saying which): |step_q32| <= 4 * 2^32, 0 <= slew_q32 <= 2^24, no flag bit outside
 * PLAY | LOOP, _pad = 0, with LOOP 0 <= loop_in < loop_out <= n_frames, and 1 <= n_frames <= 2^30. */
int mx_deck_check(const mx_deck_params* params, uint64_t n_frames);
/* Host only, pure: advance `in` by ONE tick of spt frames (1 .. MX_DECK_MAX_SPT) over a track of n_frames, with this tick's pending params / seek (or NULL): *tick is the
 * tick's record, *out the head after it (out may alias in).  The very function mx_deck_feed runs per tick.  params that mx_deck_check refuses, |in->step_q32| > 4 * 2^32,
 * spt or n_frames out of range, a NULL in / tick / out: MX_ERR_INVALID. */
int mx_deck_plan(const mx_deck_head* in, const mx_deck_params* params, const int64_t* seek_pos_q32, uint32_t spt, uint64_t n_frames, mx_deck_tick* tick, mx_deck_head* out);
/* Write the next n_ticks ticks of decks[i] into SOURCE_STEREO node nodes[i] of `g`, i < n, for the coming mx_graph_run_ticks(g, ., n_ticks): one launch for all decks
 * and ticks, on the graph's stream, into the buffer mx_graph_write_source would fill.  Asynchronous: nothing waits for the device (the per-tick descriptors go up from
 * page-locked staging that is reused only after the launch that read it has finished).  spt is the graph's.  A node that is not a SOURCE_STEREO, a bound source,
 * n_ticks = 0 or above max_ticks_per_run, a duplicate node or deck, a deck on another device, a schedule beyond n_ticks: MX_ERR_INVALID, the graph stays usable and the
 * decks stand where they stood (their schedules are dropped). */
int mx_deck_feed(mx_deck* const* decks, const uint32_t* nodes, size_t n, mx_graph* g, uint32_t n_ticks);
/* Records [first, first + n) of the deck's last feed.  Host data: no read-back, no synchronisation.  A window beyond that feed: MX_ERR_INVALID. */
int mx_deck_read_ticks(const mx_deck* d, uint32_t first, uint32_t n, mx_deck_tick* dst);
/* Where the head stands now (after the last feed). */
int mx_deck_state(const mx_deck* d, mx_deck_head* out);
/* Host only: *step_q32 = the integer nearest to speed * track_rate / graph_rate * 2^32 (exactly; ties to even): a 44 100 Hz file in a 48 000 Hz graph at speed 1 is
 * 3 946 001 203.  speed = target_bpm / the BPM mx_tempo_bpm reads.  A rate of 0, a speed that is not finite, |result| > 4 * 2^32: MX_ERR_INVALID. */
int mx_deck_step(uint32_t track_rate, uint32_t graph_rate, double speed, int64_t* step_q32);
/* Host only: bank `bank` (0 .. 3) of the coefficient tables, 257 x 32 floats. */
int mx_deck_tables(uint32_t bank, float* out);
/* DEBUG: what the last mx_deck_feed of this process launched: out[0] ticks written as zeros (not playing, BEFORE, PAST), out[1] ticks whose chunks all took the
 * streaming form (the chunk's track window staged in LDS), out[2] ticks with at least one chunk in the gather form (a loop fold or a change of direction inside the
 * chunk: taps read from the track one by one), out[3 .. 5] the same counted in chunks of MX_DECK_CHUNK frames.  Tests use it to know every form ran. */
int mx_deck_debug_last_feed(uint32_t out[6]);

/* ---- KEY-LOCK: tempo without pitch change, by overlap-add of grains placed by a waveform-similarity search (WSOLA), in integers ----
 * BUILD-SPECIFIED.  An optional rendering mode of a deck, set by mx_deck_set_keylock.  The head keeps moving exactly as mx_deck_plan says -- seek, slew, loop, clamp and
 * the tick records are what they were; params.step_q32 stays the TEMPO, the speed at which the head crosses the track.  Only what is written for a PLAYING tick changes:
 * the waveform is read in grains, each at the step pitch_q32, started wherever the head stands.  A deck that never sets key-lock is untouched in every respect.
 *
 * SETTINGS   mx_deck_keylock: 2^30 <= pitch_q32 <= 4 * 2^32 (mx_deck_step(track_rate, graph_rate, 1.0) is the original key, a factor 2^(k/12) a transposition); hop a
 *            power of two, 256 .. 8192; overlap a power of two, 16 .. min(hop / 2, 1024); radius 0 .. 1024; _pad = 0.  Recommended at 44.1 / 48 kHz: 1024 / 256 / 512
 *            (about 21 ms, 5 ms, +-11 ms).  Below: H = hop, V = overlap, R = radius, p = pitch_q32.
 * CLOCK      a key-locked deck counts its PLAYING output frames in t.  Grain j starts at t = j * H, which is some frame n of some tick of some feed; its nominal
 *            position is a_j = u'(n) of that tick (the folded position of POSITION / A TICK above).  The clock restarts -- t = 0, and grain 0 has no previous grain --
 *            at creation, at every mx_deck_set_keylock (also one that repeats the setting, and NULL), after any tick that is not playing, and when the deck is fed
 *            into another graph (another mx_graph handle) than its last feed was -- a graph that took over that graph's state with mx_graph_adopt_state is not
 *            another graph: a topology edit does not restart the clock.  A seek does NOT restart it: the cross-fade then runs from the old place to the
 *            new one, a click-free cue jump.  Neither does a change of step, a loop, nor a BEFORE / PAST tick.  All of this the host can compute.
 * POSITION   a grain with no previous grain has g_j = a_j, delta = 0, dist = 0.  Otherwise, with c = g_(j-1) + H * p (where the previous grain would continue),
 *            C = c >> 32, A = a_j >> 32 (arithmetic shifts), s[f] = L[f] + R[f] of the raw int16 track and 0 outside [0, n_frames):
 *                D(delta) = sum over i = 0 .. V - 1 of |s[C + i] - s[A + delta + i]|,   delta in [-R, R]        (at most 1024 * 131 070: it fits 32 bits)
 *            delta_j is the delta of the smallest D; ties go to the smallest |delta|, then to the negative delta.  g_j = (A + delta_j) * 2^32 + (c - C * 2^32): the grain
 *            continues c's fractional phase.  With R = 0 no search runs: delta = 0, dist = 0 (plain overlap-add).
 * OUTPUT     output frame t = j * H + m, 0 <= m < H.  G_j(m) is the deck's FILTER evaluated at u = g_j + m * p and rounded to f32 as the deck rounds it: 32 taps, the
 *            row blend, unfused f64 sums in ascending k; the taps read the track's linear neighbours and u is never folded, so a grain may read up to (H + V) * p
 *            frames past a loop's end.  The bank is chosen by the bank rule from m = p, once per setting.  If grain j has a previous grain and m < V:
 *                a = (double)G_(j-1)(H + m),  b = (double)G_j(m),  w = (double)m / (double)V,  y = (float)(a + w * (b - a)),   every operation separate;
 *            otherwise y = G_j(m).  Both channels use the same positions.  MX_DECK_TICK_BEFORE / _PAST stay in the records, but a key-locked playing tick is always
 *            rendered by this rule: zeros come out by themselves where there is no track.  A tick that is not playing is zeros.
 * IT FOLLOWS that the result does not depend on how ticks are grouped into feeds; that with p equal to a constant step (no slew, no loop fold, no seek) every c equals
 *            the next a, every delta is 0 and the output is the plain deck's bit for bit (a + w * (a - a) = a), which at unity from an integer position is the track
 *            itself; and that a negative step moves the head backwards while every grain still reads forwards.
 * RECORDS    mx_deck_grain, one per grain that STARTED in the last feed: a_q32, g_q32, the tick of the feed and the frame of that tick it starts at, delta, dist, and
 *            flags: MX_DECK_GRAIN_FIRST for a grain with no previous one.  a, tick, frame and flags are host data; g, delta and dist are computed on the device.
 * Out of scope: formant preservation, phase-vocoder stretching, grains read backwards, per-tick scheduling of key-lock settings, more than two channels.
 */
#define MX_DECK_GRAIN_FIRST 1u
typedef struct { int64_t pitch_q32; uint32_t hop; uint32_t overlap; uint32_t radius; uint32_t _pad; } mx_deck_keylock;
typedef struct { int64_t a_q32; int64_t g_q32; uint32_t tick; uint32_t frame; int32_t delta; uint32_t dist; uint32_t flags; uint32_t _pad; } mx_deck_grain;
/* Key-lock with these settings from tick 0 of the NEXT feed on; NULL: off.  Not part of the schedule: a refused feed leaves it set.  Settings that
 * mx_deck_keylock_check refuses: MX_ERR_INVALID, and the deck keeps what it had. */
int mx_deck_set_keylock(mx_deck* d, const mx_deck_keylock* k);
/* Host only: the SETTINGS rules alone. */
int mx_deck_keylock_check(const mx_deck_keylock* k);
/* Host only, pure: the search rule of POSITION alone, in plain C++ -- *delta and *dist for a previous grain continuing at frame C and a nominal frame A, over a track of
 * n_frames interleaved stereo frames.  overlap 1 .. 1024 (any value, not only the powers of two a setting may have), radius 0 .. 1024 (0: the one candidate's D),
 * |C|, |A| <= 2^40.  Anything else, a NULL pointer, n_frames outside 1 .. 2^30: MX_ERR_INVALID. */
int mx_deck_keylock_search(const int16_t* interleaved, uint64_t n_frames, int64_t C, int64_t A, uint32_t overlap, uint32_t radius, int32_t* delta, uint32_t* dist);
/* How many grains started in the deck's last feed (0 for a plain deck).  Host data: no synchronisation. */
int mx_deck_grain_count(const mx_deck* d, uint32_t* n);
/* Grain records [first, first + n) of the last feed.  THE ONE CALL OF THE DECK THAT WAITS for the feed's kernels (g, delta and dist come back from the device); it is
 * indication only and never needed to play.  A window beyond the last feed's grains: MX_ERR_INVALID. */
int mx_deck_read_grains(mx_deck* d, uint32_t first, uint32_t n, mx_deck_grain* dst);
/* DEBUG: the key-locked decks of the last mx_deck_feed of this process: out[0] grains placed by a search, out[1] grains without one (a first grain, or radius 0),
 * out[2] render chunks (MX_DECK_CHUNK frames of a playing tick) with at least one fading lane, out[3] render chunks with a grain start after their first lane.
 * mx_deck_debug_last_feed counts the plain decks of the feed only. */
int mx_deck_debug_last_keylock(uint32_t out[4]);

/* ---- ECHO: a beat-synced feedback delay behind the deck, with echo-out ----
 * BUILD-SPECIFIED.  An optional pass of a deck, set by mx_deck_set_echo / mx_deck_schedule_echo: a recursive delay line per deck that runs in place on what the deck
 * wrote into its SOURCE_STEREO node's port, by the plain deck's rule or by key-lock's -- the echo does not look at how those samples were made.  The head, the tick
 * records and the grains are what they were.  A deck that never sets an echo is untouched in every respect, and a feed in which no deck has an echo launches nothing new.
 *
 * SETTINGS   mx_deck_echo: MX_DECK_ECHO_MIN_DELAY <= delay <= MX_DECK_ECHO_MAX_DELAY output frames (mx_deck_echo_delay turns a beat fraction into one); send, feedback,
 *            wet and damp finite, |send| <= 1, |feedback| <= 1, |wet| <= 4, 0 <= damp <= 1; no flag bit other than MX_DECK_ECHO_PINGPONG.
 * CLOCK      a deck with an echo counts EVERY output frame it is fed in t: playing ticks, ticks written as zeros (not playing), BEFORE / PAST ticks.  That is how a
 *            stopped deck rings out.  The delay line r_c[s], one per channel c, holds what PER FRAME wrote at clock s.  t = 0 and an all-zero line (r_c[s] = 0 for
 *            every s < 0) hold at the first tick that runs with an echo after creation or after a tick without one: off -> on starts clean.  Nothing else restarts
 *            the clock or clears the line: not a seek, a load, a change of step or of PLAY, a change of settings (a change of delay included: the new delay reads the
 *            line the old one wrote), mx_deck_set_keylock, a feed into another graph handle, nor a graph that adopted another's state.  All of this the host can compute.
 * PER FRAME  x_c[t] is the f32 the deck wrote for channel c (0 = L, 1 = R) at the frame with clock t.  c' is the other channel under MX_DECK_ECHO_PINGPONG, else c.
 *            D is the tick's delay, s = t - D.  Every multiply and add is a separate f64 operation, never fused, in this order:
 *                a = (double)damp * 0.25;   b = 1.0 - (a + a)                                              (per setting)
 *                f_c = b * (double)r_c'[s] + a * (double)r_c'[s - 1] + a * (double)r_c'[s + 1]             (left to right: ((b r) + (a r)) + (a r); with damp = 0, r_c'[s])
 *                r_c[t] = (float)((double)send_n * (double)x_c[t] + (double)fb_n * f_c)
 *                y_c[t] = (float)((double)x_c[t] + (double)wet_n * f_c)
 *            y replaces x in the port.  Subnormal f32 values are kept, not flushed (numpy's casts are the model).  MX_FLAG_FP_CONTRACT does not apply.  s + 1 <= t - 255:
 *            a frame never reads what it or a later frame writes.
 * RAMPS      send, feedback and wet never jump inside the sound.  In the tick at which a setting takes effect (any mx_deck_set_echo / mx_deck_schedule_echo with
 *            settings, also one that repeats them), frame n of the tick, n = 0 .. spt - 1, uses for each of the three
 *                g_n = (float)((double)old + ((double)new - (double)old) * ((double)n / (double)spt))
 *            with `old` the value of the tick before (0 in the first tick after off -> on); every other tick uses `new` as it stands.  delay, damp and the flag
 *            switch at the tick's first frame.
 * SCHEDULE   mx_deck_set_echo applies from tick 0 of the next feed, mx_deck_schedule_echo from the tick named; NULL settings turn the echo off from that tick.  The
 *            rules are mx_deck_schedule's: a later call for the same tick replaces an earlier one, the feed clears the schedule, a feed that does not reach a
 *            scheduled tick fails with MX_ERR_INVALID and drops the schedule (the deck's own too) -- the setting in force, the clock and the line stay.
 * IT FOLLOWS that the result does not depend on how ticks are grouped into feeds; that with wet = 0 the port holds the deck's own samples; that with send = 0,
 *            feedback = 1, damp = 0 the line recirculates bit for bit for ever (the freeze; f_c = r_c'[s] then as a number, a -0 may come back as +0); that without
 *            PINGPONG the two channels never meet; and that a deck whose PLAY flag is cleared keeps sounding its tail (the echo-out).
 * BLOCKS     (how the device runs it; mx_deck_echo_plan restates it.)  Frame t reads the line no later than t - D + 1, so the frames of a block [t0, t0 + B) are
 *            independent of one another when t - D(t) + 1 < t0 for every frame of it; with one delay, B <= D - 1.  A deck's echo frames of a feed are cut greedily
 *            into maximal such blocks, a tick without an echo always ending one; the cut holds across a tick that lowers the delay.
 * Out of scope: delays under 256 frames (flanger, chorus), modulated or interpolated delay, the echo on ports other than a deck's
 * source, more than two channels.  (The reverb is REVERB below: a pass of its own behind the echo.)
 */
#define MX_DECK_ECHO_PINGPONG 1u
#define MX_DECK_ECHO_MIN_DELAY 256u
#define MX_DECK_ECHO_MAX_DELAY 262144u      /* 5.4 s at 48 kHz */
typedef struct { uint32_t delay; uint32_t flags; float send; float feedback; float wet; float damp; } mx_deck_echo;   /* 24 bytes */
/* The echo with these settings from tick 0 of the NEXT feed on; NULL: off from that tick.  mx_deck_schedule_echo(d, 0, e).  The first call with settings allocates the
 * deck's delay line (2^19 frames, 4 MB).  Settings that mx_deck_echo_check refuses: MX_ERR_INVALID, and the deck and its schedule keep what they had. */
int mx_deck_set_echo(mx_deck* d, const mx_deck_echo* e);
/* ... from tick `tick_in_feed` of the next feed on (SCHEDULE). */
int mx_deck_schedule_echo(mx_deck* d, uint32_t tick_in_feed, const mx_deck_echo* e);
/* Host only: the SETTINGS rules alone. */
int mx_deck_echo_check(const mx_deck_echo* e);
/* mx_deck_echo_delay (host only: the delay of num / den beats) is declared below mx_deck_sync, with the mx_deck_beats it reads. */
/* After the last feed: the clock t, whether the echo is on (1 / 0), and the setting in force (the last one it had, when off; all zero before the first).  Host data: no
 * synchronisation. */
int mx_deck_echo_state(const mx_deck* d, uint64_t* t, uint32_t* on, mx_deck_echo* setting);
/* Host only, pure: BLOCKS for a feed of n_ticks ticks of spt frames, delay[k] the delay of tick k or 0 for a tick without an echo: block j is blocks[2 j] (its first
 * frame, counted from the feed's first) and blocks[2 j + 1] (its frames), for j < min(*n_blocks, cap); *n_blocks is the number of blocks whatever cap is.  spt outside
 * 1 .. MX_DECK_MAX_SPT, a delay that is neither 0 nor within MIN .. MAX, a NULL pointer: MX_ERR_INVALID. */
int mx_deck_echo_plan(uint32_t spt, const uint32_t* delay, uint32_t n_ticks, uint64_t* blocks, uint32_t cap, uint32_t* n_blocks);
/* DEBUG: the decks with an echo in any tick of the last mx_deck_feed of this process: out[0] decks rendered in the one-block form (the deck's echo frames of the feed are
 * a single block: a lane per frame, no barrier), out[1] decks in the sequential form (one workgroup walks the deck's blocks in order), out[2] the blocks those walked,
 * out[3] those of them that cross a tick boundary.  All zero for a feed in which no deck has an echo. */
int mx_deck_debug_last_echo(uint32_t out[4]);

/* ---- FILTER: a resonant sweep filter behind the deck, ahead of the echo ----
 * BUILD-SPECIFIED.  An optional pass of a deck, set by mx_deck_set_filter / mx_deck_schedule_filter: the one-knob filter of a transition, a trapezoidal
 * (topology-preserving) state-variable filter of second order whose one core gives low-pass, high-pass, band-pass and notch, and which stays stable while its
 * coefficients move -- a sweep is nothing but moving coefficients.  It runs in place on what the deck wrote into its SOURCE_STEREO node's port, by the plain deck's
 * rule or by key-lock's, and the echo behind it (ECHO above) reads the filtered samples: the order is feed / key-lock -> filter -> echo, so an echo-out under a
 * closing low-pass sends the filtered sound down the line, and the tail already in the line is not filtered again.  The head, the tick records and the grains are
 * what they were.  A deck that never sets a filter is untouched in every respect, and a feed in which no deck has a filter launches nothing new and uploads no
 * further byte.
 *
 * SETTINGS   mx_deck_filter: kind one of MX_DECK_FILTER_LP / HP / BP / NOTCH; g = tan(pi fc / rate) with MX_DECK_FILTER_MIN_G (2^-12) <= g <= MX_DECK_FILTER_MAX_G
 *            (16); k = 1 / Q with MX_DECK_FILTER_MIN_K (0.05) <= k <= MX_DECK_FILTER_MAX_K (2); 0 <= wet <= 1; all three finite; flags and _pad 0.  The bounds are
 *            compared as f32 (0.05 is the f32 nearest to it).  mx_deck_filter_design turns a cutoff and a Q into g and k, mx_deck_filter_knob a DJ knob into both.
 * STATE      four f64 values per deck, s1 and s2 of L, then s1 and s2 of R, in device memory the deck owns (32 bytes, allocated at the first setting).  All four
 *            are zero at the first tick that runs with a filter after creation or after a tick without one: off -> on starts clean.  Nothing else clears them: not
 *            a seek, a load, a change of PLAY, of step or of settings (a change of kind included), mx_deck_set_keylock, an echo setting, a feed into another graph
 *            handle, nor a graph that adopted another's state.  The filter runs on EVERY frame the deck is fed while it is on: playing ticks, ticks written as
 *            zeros (not playing), BEFORE / PAST ticks.  That is how a stopped deck's resonance rings out.
 * PER FRAME  the tick has spt frames.  For frame n of the tick, n = 0 .. spt - 1, and channel c, x = (double) of the f32 the deck wrote.  Every multiply, add and
 *            divide is a separate f64 operation, never fused, in exactly this order and association:
 *                w  = (double)n / (double)spt                                          (ramp ticks only, see RAMPS)
 *                gn = g_old + (g_new - g_old) * w                                      (f64 throughout, g_old and g_new the f32 settings widened; a tick
 *                kn = k_old + (k_new - k_old) * w                                       without a ramp: gn = (double)g_new, kn = (double)k_new,
 *                wn = wet_old + (wet_new - wet_old) * w                                 wn = (double)wet_new)
 *                d  = 1.0 + gn * (gn + kn);   a1 = 1.0 / d;   a2 = gn * a1;   a3 = gn * a2
 *                v3 = x - s2
 *                v1 = a1 * s1 + a2 * v3
 *                v2 = s2 + (a2 * s1 + a3 * v3)
 *                s1 = (v1 + v1) - s1;   s2 = (v2 + v2) - s2
 *                f  = LP: v2    BP: v1    HP: (x - kn * v1) - v2    NOTCH: x - kn * v1
 *                y  = (float)(x + wn * (f - x))
 *            y replaces x in the port; s1 and s2 are the channel's own.  Subnormal f32 values are kept, not flushed (numpy's casts are the model), and the f64
 *            division is the correctly rounded one.  MX_FLAG_FP_CONTRACT does not apply.
 * RAMPS      g, k and wet never jump inside the sound.  In the tick at which a setting takes effect (any mx_deck_set_filter / mx_deck_schedule_filter with settings,
 *            also one that repeats them), the three go from the values of the tick before (`old`) to the new ones by the formulas above; in the first tick after
 *            off -> on, g_old = g_new, k_old = k_new and wet_old = 0: a fade-in at the target cutoff, not a sweep from nowhere.  Every other tick uses the new
 *            values as they stand.  kind switches at the tick's first frame.  Turning the filter off is a hard switch at a tick's first frame; a host that wants a
 *            smooth exit schedules wet = 0 one tick earlier.  (In a tick of one frame w is always 0: the tick sounds the old values whole.)
 * SCHEDULE   mx_deck_set_filter applies from tick 0 of the next feed, mx_deck_schedule_filter from the tick named; NULL settings turn the filter off from that
 *            tick.  The rules are mx_deck_schedule_echo's: a later call for the same tick replaces an earlier one, the feed clears the schedule, a feed that does
 *            not reach a scheduled tick fails with MX_ERR_INVALID and drops the schedules (the deck's own and the echo's too) -- the setting in force and the state
 *            stay.  Settings that mx_deck_filter_check refuses leave everything as it was.
 * IT FOLLOWS that the result does not depend on how ticks are grouped into feeds; that with wet = 0 the port holds the deck's own samples as numbers (y =
 *            (float)(x + 0 * (f - x)): a -0 may come back as +0) while the state moves on all the same; that the two channels never meet; that the kind can change
 *            without touching the state (s1 and s2 do not depend on it); and that a deck whose PLAY flag is cleared keeps ringing.
 * Out of scope: a time-parallel, not bit-exact form of the recurrence; filters of other orders; drive or saturation; the filter on ports other than a deck's source;
 * more than two channels; per-frame automation finer than the per-tick ramp.
 */
#define MX_DECK_FILTER_LP 0u
#define MX_DECK_FILTER_HP 1u
#define MX_DECK_FILTER_BP 2u
#define MX_DECK_FILTER_NOTCH 3u
#define MX_DECK_FILTER_MIN_G 0.000244140625f   /* 2^-12: 3.7 Hz at 48 kHz */
#define MX_DECK_FILTER_MAX_G 16.0f             /* 0.48 of the rate */
#define MX_DECK_FILTER_MIN_K 0.05f             /* Q = 20 */
#define MX_DECK_FILTER_MAX_K 2.0f              /* Q = 1 / 2: two real poles at the same place */
typedef struct { uint32_t kind; uint32_t flags; float g; float k; float wet; uint32_t _pad; } mx_deck_filter;   /* 24 bytes */
/* What mx_deck_filter_host carries from one call to the next: the four state values (STATE's order), the last setting, whether the filter was on (1 / 0); _pad 0.
 * All zero is a deck that never had a filter. */
typedef struct { double s[4]; mx_deck_filter last; uint32_t on; uint32_t _pad; } mx_deck_filter_carry;   /* 64 bytes */
/* The filter with these settings from tick 0 of the NEXT feed on; NULL: off from that tick.  mx_deck_schedule_filter(d, 0, f).  The first call with settings allocates
 * the deck's state (32 bytes).  Settings that mx_deck_filter_check refuses: MX_ERR_INVALID, and the deck and its schedule keep what they had. */
int mx_deck_set_filter(mx_deck* d, const mx_deck_filter* f);
/* ... from tick `tick_in_feed` of the next feed on (SCHEDULE). */
int mx_deck_schedule_filter(mx_deck* d, uint32_t tick_in_feed, const mx_deck_filter* f);
/* Host only: the SETTINGS rules alone. */
int mx_deck_filter_check(const mx_deck_filter* f);
/* After the last feed: whether the filter is on (1 / 0) and the setting in force (the last one it had, when off; all zero before the first).  Host data: no
 * synchronisation. */
int mx_deck_filter_state(const mx_deck* d, uint32_t* on, mx_deck_filter* setting);
/* Waits for the feed's kernels, then: the four state values as they stand after the last feed, in STATE's order -- or all zeros when the filter is off or was never on. */
int mx_deck_read_filter_state(mx_deck* d, double s[4]);
/* Host only: *out = { kind, 0, (float)tan(pi cutoff_hz / rate), (float)(1 / q), (float)wet, 0 }.  Uses libm: specified to 1 f32 ulp, not to the bit -- the bit-exact
 * path starts at mx_deck_filter.  An argument that is not finite, rate or q not positive, a cutoff outside (0, rate / 2), or a result that mx_deck_filter_check
 * refuses: MX_ERR_INVALID, *out untouched. */
int mx_deck_filter_design(uint32_t kind, double cutoff_hz, double q, double rate, double wet, mx_deck_filter* out);
/* Host only: the DJ mapping of one knob in -1 .. 1, on mx_deck_filter_design.  |knob| < 1/64: *on = 0, *out untouched (the dead zone: no filter).  knob in [-1, 0):
 * *on = 1, a low-pass at 20000 (80 / 20000)^|knob| Hz; knob in (0, 1]: *on = 1, a high-pass at 20 (8000 / 20)^knob Hz; the cutoff no higher than 0.45 rate; wet 1.
 * A knob outside -1 .. 1 or not finite, and what mx_deck_filter_design refuses: MX_ERR_INVALID. */
int mx_deck_filter_knob(double knob, double rate, double q, mx_deck_filter* out, uint32_t* on);
/* Host only, pure: PER FRAME and RAMPS in plain C++ over the caller's frames[n_ticks * spt * 2] (L R interleaved), in place.  settings[k] is the setting in force in
 * tick k, NULL for a tick without a filter; every tick with a setting counts as one at which that setting takes effect (a setting that repeats the last ramps from
 * equal values, which is the constant tick bit for bit).  *carry goes in as the last call left it (all zero at first) and comes out as this call leaves it; its s[] is
 * zero when the last tick had no filter.  spt outside 1 .. MX_DECK_MAX_SPT, a setting or carried block the check refuses, NULL: MX_ERR_INVALID, nothing written. */
int mx_deck_filter_host(float* frames, uint32_t spt, uint32_t n_ticks, const mx_deck_filter* const* settings, mx_deck_filter_carry* carry);
/* DEBUG: the decks with a filter in any tick of the last mx_deck_feed of this process: out[0] those decks, out[1] their ticks with a ramp, out[2] their ticks with a
 * filter and no ramp, out[3] the 64-frame super-blocks their waves walked (ceil(n_ticks spt / 64) per deck: the walk covers the feed).  All zero for a feed in which
 * no deck has a filter. */
int mx_deck_debug_last_filter(uint32_t out[4]);

/* ---- REVERB: a feedback delay network behind the deck, the filter and the echo, with reverb-out ----
 * BUILD-SPECIFIED.  An optional pass of a deck, set by mx_deck_set_reverb / mx_deck_schedule_reverb: the wash of a transition.  Two series allpass diffusers per
 * channel feed a tank of eight delay lines mixed by an orthogonal (Hadamard) matrix.  It runs LAST, in place on what the deck, the filter and the echo left in the
 * deck's SOURCE_STEREO node's port: feed / key-lock -> filter -> echo -> reverb, so echo repeats are reverberated.  The head, the tick records and the grains are
 * what they were.  A deck that never sets a reverb is untouched in every respect, and a feed in which no deck has a reverb launches nothing new and uploads no
 * further byte.
 *
 * SETTINGS   mx_deck_reverb: delay[i], i = 0 .. 7, the tank line delays in output frames, MX_DECK_REVERB_MIN_DELAY (128) <= delay[i] <= MX_DECK_REVERB_MAX_DELAY
 *            (12000); diff[j], j = 0 .. 3, the diffuser delays, MX_DECK_REVERB_MIN_DIFF (64) <= diff[j] <= MX_DECK_REVERB_MAX_DIFF (2000): diff[0] then diff[1]
 *            serve L in series, diff[2] then diff[3] serve R.  All floats finite; |gain[i]| <= 1, |send| <= 1, |dry| <= 1, |wet| <= 4, 0 <= damp <= 1,
 *            0 <= diffusion <= 0.75 (compared as f32); flags 0.  mx_deck_reverb_design turns a size and a decay time into one.
 * MEMORY     per deck, allocated at the first setting: eight tank rings r_i of MX_DECK_REVERB_TANK_RING (16384) f32 and four diffuser rings q_j of
 *            MX_DECK_REVERB_DIFF_RING (4096) f32, one ring a line, one after another (MX_DECK_REVERB_LINE_FLOATS = 147456 f32, 576 KB): ring i of the tank starts
 *            at float i * 16384, ring j of the diffusers at float 8 * 16384 + j * 4096.  The value of clock s lies in slot s & (ring - 1).  A read at a clock below
 *            0 is zero, whatever the slot holds: off -> on needs no clearing.  The longest block (BLOCKS) plus the longest delay plus one stays under the ring,
 *            2000 + 12000 + 1 < 16384 and 2000 + 2000 < 4096, so no frame of a block overwrites a slot another frame of that block still reads.
 * CLOCK      the echo's rule.  A deck with a reverb counts EVERY output frame it is fed in t: playing ticks, ticks written as zeros (not playing), BEFORE / PAST
 *            ticks.  That is how a stopped deck rings out.  t = 0 and all-zero lines (every read below clock 0) hold at the first tick that runs with a reverb
 *            after creation or after a tick without one: off -> on starts clean.  Nothing else restarts the clock or clears the lines: not a seek, a load, a change
 *            of step or of PLAY, a change of settings (delays included: the new delay reads what the old one wrote), mx_deck_set_keylock, a filter or echo
 *            setting, a feed into another graph handle, nor a graph that adopted another's state.  All of this the host can compute.
 * PER FRAME  x_c is the f32 in the port for channel c (0 = L, 1 = R) at the frame with clock t: what the deck, the filter and the echo left there.  send_n, dry_n,
 *            wet_n, gain_n[i] are the frame's ramped values (RAMPS), each an f32 widened.  Every multiply, add and subtract is a separate f64 operation, never
 *            fused, in this order:
 *             1. a = (double)damp * 0.25;   b = 1.0 - (a + a);   gd = (double)diffusion                                   (per setting)
 *             2. u = send_n * x_c
 *             3. for j = 2c, then 2c + 1, with p = (double)q_j[t - diff_j]:
 *                    v = u - gd * p;   q_j[t] = (float)v;   w = (double)(float)v;   u = p + gd * w
 *                after both, e_c = u.  The rounded w is used, not v: the allpass is allpass with respect to what the line holds.
 *             4. for i = 0 .. 7, s = t - delay_i:
 *                    f_i = b * (double)r_i[s] + a * (double)r_i[s - 1] + a * (double)r_i[s + 1]         (left to right: ((b r) + (a r)) + (a r))
 *                    g_i = gain_n[i] * f_i
 *             5. h = g; three stages at distances d = 1, 2, 4: for every i with bit d clear, (h_i, h_{i+d}) <- (h_i + h_{i+d}, h_i - h_{i+d}), both from the
 *                stage's inputs.  Then m_i = h_i * C, C = 0x1.6a09e667f3bcdp-2 (the f64 nearest 0.5 sqrt(0.5)).
 *             6. r_i[t] = (float)(m_i + e_{i & 1})                                                        (even lines take L, odd lines R)
 *             7. o_0 = ((f_0 - f_2) + (f_4 - f_6)) * 0.5;   o_1 = ((f_1 - f_3) + (f_5 - f_7)) * 0.5
 *                y_c = (float)(dry_n * x_c + wet_n * o_c)
 *            y replaces x in the port.  Subnormal f32 values are kept, not flushed (numpy's casts are the model).  MX_FLAG_FP_CONTRACT does not apply.  A frame
 *            reads r_i no later than clock t - 127 and q_j no later than t - 64: never what it or a later frame writes.
 * RAMPS      send, dry, wet and the eight gains never jump inside the sound.  In the tick at which a setting takes effect (any mx_deck_set_reverb /
 *            mx_deck_schedule_reverb with settings, also one that repeats them), frame n of the tick, n = 0 .. spt - 1, uses for each of the eleven
 *                g_n = (float)((double)old + ((double)new - (double)old) * ((double)n / (double)spt))
 *            with `old` the value of the tick before; every other tick uses `new` as it stands.  In the first tick after off -> on `old` is 0 for ALL eleven,
 *            dry included: that tick fades the dry signal in from silence too (a host that wants the dry signal untouched at the switch-on sets the reverb a
 *            tick early with send = 0, or keeps dry at 1 by switching on under a tick of silence).  delay, diff, damp and diffusion switch at the tick's first
 *            frame.  Turning the reverb off is a hard switch at a tick's first frame.  (In a tick of one frame the weight is always 0: the tick sounds the old
 *            values whole.)
 * SCHEDULE   mx_deck_set_reverb applies from tick 0 of the next feed, mx_deck_schedule_reverb from the tick named; NULL settings turn the reverb off from that
 *            tick.  The rules are mx_deck_schedule_echo's: a later call for the same tick replaces an earlier one, the feed clears the schedule, a feed that does
 *            not reach a scheduled tick fails with MX_ERR_INVALID and drops the schedules (the deck's own, the filter's and the echo's too) -- the setting in
 *            force, the clock and the lines stay.  Settings that mx_deck_reverb_check refuses leave everything as it was.
 * BLOCKS     (how the device runs it; mx_deck_reverb_plan restates it.)  The reach of a tick is R = min(min_i delay_i - 1, min_j diff_j), 64 <= R <= 2000: frame
 *            t reads no line later than clock t - R.  The frames of a block [t0, t0 + B) are independent of one another when t - R(t) < t0 for every frame of it;
 *            with one setting, B <= R.  A deck's reverb frames of a feed are cut greedily into maximal such blocks, a tick without a reverb always ending one;
 *            the cut holds across a tick that lowers the reach.
 * IT FOLLOWS that the result does not depend on how ticks are grouped into feeds; that with wet = 0 and dry = 1 the port holds the deck's samples as numbers
 *            ((float)(1 * x + 0 * o): a -0 may come back as +0) while the lines move on; that with all gain = 0 and diffusion = 0 the wet signal is a four-tap
 *            delay of the sent input that can be written down from the port alone: a diffuser with diffusion = 0 is a pure delay of diff_j frames, so with
 *            u_c[t] = (double)(float)(send_t' * x_c[t']) at t' = t - diff_2c - diff_2c+1 (zero for t' < 0) and damp = 0,
 *            o_0[t] = 0.5 ((u_0[t - D0] - u_0[t - D2]) + (u_0[t - D4] - u_0[t - D6])), and likewise o_1 with the odd delays; and that a deck whose PLAY flag is
 *            cleared keeps sounding its tail (the reverb-out).
 * Out of scope: pre-delay; modulated or interpolated lines; a one-pole damping (it would serialise the block); a bit-exact freeze (orthogonal mixing in floating
 * point holds energy only within rounding); the reverb on ports other than a deck's source; more than two channels.
 */
#define MX_DECK_REVERB_MIN_DELAY 128u
#define MX_DECK_REVERB_MAX_DELAY 12000u     /* 250 ms at 48 kHz */
#define MX_DECK_REVERB_MIN_DIFF 64u
#define MX_DECK_REVERB_MAX_DIFF 2000u
#define MX_DECK_REVERB_TANK_RING 16384u
#define MX_DECK_REVERB_DIFF_RING 4096u
#define MX_DECK_REVERB_LINE_FLOATS 147456u  /* 8 x 16384 + 4 x 4096 */
typedef struct { uint32_t delay[8]; uint32_t diff[4]; float gain[8]; float send; float dry; float wet; float damp; float diffusion; uint32_t flags; } mx_deck_reverb;   /* 104 bytes */
/* What mx_deck_reverb_host carries from one call to the next beside the caller's lines: the clock t, the last setting, whether the reverb was on (1 / 0); _pad 0.
 * All zero is a deck that never had a reverb. */
typedef struct { uint64_t t; mx_deck_reverb last; uint32_t on; uint32_t _pad; } mx_deck_reverb_carry;   /* 120 bytes */
/* The reverb with these settings from tick 0 of the NEXT feed on; NULL: off from that tick.  mx_deck_schedule_reverb(d, 0, r).  The first call with settings allocates
 * the deck's lines (MEMORY, 576 KB).  Settings that mx_deck_reverb_check refuses: MX_ERR_INVALID, and the deck and its schedule keep what they had. */
int mx_deck_set_reverb(mx_deck* d, const mx_deck_reverb* r);
/* ... from tick `tick_in_feed` of the next feed on (SCHEDULE). */
int mx_deck_schedule_reverb(mx_deck* d, uint32_t tick_in_feed, const mx_deck_reverb* r);
/* Host only: the SETTINGS rules alone. */
int mx_deck_reverb_check(const mx_deck_reverb* r);
/* After the last feed: the clock t, whether the reverb is on (1 / 0), and the setting in force (the last one it had, when off; all zero before the first).  Host data:
 * no synchronisation. */
int mx_deck_reverb_state(const mx_deck* d, uint64_t* t, uint32_t* on, mx_deck_reverb* setting);
/* Waits for the feed's kernels, then: the raw rings into dst[MX_DECK_REVERB_LINE_FLOATS], tank then diffusers (MEMORY's layout).  Only the slots of the clocks in
 * [max(0, t - ring), t) are specified; all zeros for a deck that never had a setting. */
int mx_deck_read_reverb_lines(mx_deck* d, float* dst);
/* Host only, pure: BLOCKS for a feed of n_ticks ticks of spt frames, settings[k] the setting in force in tick k or NULL for a tick without a reverb: block j is
 * blocks[2 j] (its first frame, counted from the feed's first) and blocks[2 j + 1] (its frames), for j < min(*n_blocks, cap); *n_blocks is the number of blocks
 * whatever cap is.  spt outside 1 .. MX_DECK_MAX_SPT, a setting the check refuses, a NULL pointer: MX_ERR_INVALID. */
int mx_deck_reverb_plan(uint32_t spt, const mx_deck_reverb* const* settings, uint32_t n_ticks, uint64_t* blocks, uint32_t cap, uint32_t* n_blocks);
/* Host only, pure: PER FRAME, RAMPS and CLOCK in plain C++ over the caller's frames[n_ticks * spt * 2] (L R interleaved), in place, and the caller's
 * lines[MX_DECK_REVERB_LINE_FLOATS] (MEMORY's layout; any content at first).  settings[k] is the setting in force in tick k, NULL for a tick without a reverb; every
 * tick with a setting counts as one at which that setting takes effect (a setting that repeats the last ramps from equal values, which is the constant tick bit for
 * bit).  *carry goes in as the last call left it (all zero at first) and comes out as this call leaves it.  spt outside 1 .. MX_DECK_MAX_SPT, a setting or carried
 * block the check refuses, NULL: MX_ERR_INVALID, nothing written. */
int mx_deck_reverb_host(float* frames, uint32_t spt, uint32_t n_ticks, const mx_deck_reverb* const* settings, float* lines, mx_deck_reverb_carry* carry);
/* Host only: knobs into a setting.  size in 0.25 .. 4 scales the room, t60_seconds > 0 is the time the tank takes to fall by 60 dB, rate > 0 the graph's rate; all
 * finite.  With P(x) the smallest prime >= x and the f64 expressions evaluated left to right as written:
 *   tank     delay[i] = P(floor(base[i] * size * rate / 48000.0 + 0.5)), base = {1087, 1283, 1447, 1663, 1871, 2053, 2281, 2477}, for i = 0 .. 7 in turn; while the
 *            prime equals a delay already given to a lower i, the next prime above it is taken
 *   diffuser diff[j] = P(floor(dbase[j] * rate / 48000.0 + 0.5)), dbase = {229, 613, 241, 587}
 *   gain[i] = (float)pow(10.0, -3.0 * (double)delay[i] / (rate * t60_seconds))        (libm: specified to 1 f32 ulp, not to the bit; the integers are exact)
 *   send, dry, wet, damp, diffusion as given, rounded to f32; flags 0.
 * An argument that is not finite, size outside 0.25 .. 4, rate or t60_seconds not positive, a delay out of range or a result that mx_deck_reverb_check refuses:
 * MX_ERR_INVALID, *out untouched. */
int mx_deck_reverb_design(double rate, double size, double t60_seconds, double damp, double diffusion, double send, double dry, double wet, mx_deck_reverb* out);
/* DEBUG: the decks with a reverb in any tick of the last mx_deck_feed of this process: out[0] those decks, out[1] the blocks their workgroups walked, out[2] those of
 * them that cross a tick boundary, out[3] the frames of the largest block.  All zero for a feed in which no deck has a reverb. */
int mx_deck_debug_last_reverb(uint32_t out[4]);

/* ---- ANALYSIS: the band waveform overview, the onset autocorrelation and the beat grid of a whole track, before it sounds ----
 * BUILD-SPECIFIED.  One pass over the track as it lies in device memory, on the deck's own load stream: what a host needs at load time -- the coloured overview
 * (low / mid / high per column), the tempo, and where the beats are.  Everything up to the read-out of the beat grid is integer arithmetic, so no order of accumulation
 * matters and the records are fixed count for count.  A deck that never calls mx_deck_analyse is untouched in every respect.
 *
 * SETTINGS   mx_deck_analysis: column C a power of two, 64 .. 4096 frames; taps K odd, 1 .. 127; max_lag L 16 .. 1024; _pad 0; lo[0 .. K) and hi[0 .. K) two low-pass
 *            tap tables in Q14, each with sum |c_k| <= 32767, entries at index K and above 0.  mx_deck_analysis_check enforces exactly these rules.
 *            mx_deck_analysis_bands fills the tables (TABLES); worth starting from: 200 Hz / 2.5 kHz, K = 63, C = 512, L = 256.
 * SIGNAL     s[f] = L[f] + R[f] of the raw int16 track, 0 outside [0, n_frames) (key-lock's s; |s| <= 65536).  With D = (K - 1) / 2:
 *                a1[f] = sum_k lo[k] s[f - D + k],   a2[f] = sum_k hi[k] s[f - D + k]      (|a| <= 65536 * 32767 < 2^31: int32 is exact -- why the tap rule is what it is)
 *                low[f] = a1[f] >> 14,  b[f] = a2[f] >> 14  (arithmetic shifts: floor),  mid[f] = b[f] - low[f],  high[f] = s[f] - b[f]
 *            so low + mid + high = s for every frame, exactly.
 * COLUMNS    N = ceil(n_frames / C).  Column c covers the frames f of [c C, (c + 1) C) with f < n_frames; the last may be short, and frames beyond the track contribute
 *            to nothing.  mx_deck_column, 56 bytes: smin, smax the extremes of s over the column; peak[3] = max |band| for low, mid, high; energy[3] = sum band^2;
 *            e = sum s^2 (at most 2^44); onset as below.
 * ONSET      the tempo taps' rule: A[c] = floor(sqrt(e[c])), the exact integer root, A[-1] = 0; onset[c] = max(A[c] - A[c - 1], 0) >> 6 (<= 2^16).
 * AUTOCORR   for l = 0 .. L - 1: R[l] = sum_{c = 0}^{N - 1 - l} onset[c] onset[c + l] as uint64 (0 when l >= N; at most 2^32 * 2^24: no overflow).
 * BEAT GRID  mx_deck_beatgrid, host only and pure.  The lag follows EXACTLY mx_tempo_bpm's rule with C in place of hop_frames: the candidate lags are the integers of
 *            [60 rate / (C bpm_hi), 60 rate / (C bpm_lo)] within [1, L - 2], l* the first maximum of R over them, d that function's parabolic term.  P = (double)l* + d.
 *            For phi = 0 .. ceil(P) - 1: S(phi) = sum_{k = 0, 1, ...} onset[i_k] as uint64, i_k = (int64)floor((double)phi + (double)k * P) while i_k < n_cols -- the
 *            multiply and the add separate f64 operations, never fused.  The phase is the smallest phi of the largest S.  mx_deck_grid: bpm = 60 rate / (C P),
 *            period_columns = P, confidence = R[l*] / R[0], first_beat_frame = phi C, lag = l*, phase_column = phi; beat j lies near frame (phi + j P) C.
 *            With R[0] = 0 or no candidate lag everything is 0 -- and also when P lies outside [1, L]: the vertex of the parabola runs away only from a "maximum" at
 *            the edge of the candidate range whose neighbour outside the range is larger, and such a period places no beats.
 * TABLES     mx_deck_analysis_bands: Hann-windowed sincs at cutoffs f_lo < f_hi < rate / 2.  g_k = fc sinc(fc (k - D)) w_k, fc = 2 f / rate, sinc(x) = sin(pi x) / (pi x),
 *            w_k = 0.5 - 0.5 cos(2 pi (k + 1) / (K + 1)), evaluated in f64 for k <= D and mirrored; each tap the nearest integer of 16384 g_k / sum g; the centre tap then
 *            adjusted so that sum c = 16384 exactly: DC passes at gain 1, and a constant track has mid = high = 0 away from its ends.
 * Out of scope: gated-loudness (LUFS) auto-gain and whole-track key (the columns' e and peaks serve a plain gain; key can follow on the same pass); tempo that changes
 * within a track; downbeat / bar detection (BARS below has it); analysis of a range instead of the whole track; more than two channels; any change to how a deck plays. */
typedef struct { uint32_t column; uint32_t taps; uint32_t max_lag; uint32_t _pad; int16_t lo[127]; int16_t hi[127]; } mx_deck_analysis;
typedef struct { int32_t smin, smax; uint32_t peak[3]; uint32_t onset; uint64_t energy[3]; uint64_t e; } mx_deck_column;
typedef struct { double bpm, period_columns, confidence; uint64_t first_beat_frame; uint32_t lag, phase_column; } mx_deck_grid;
/* Host only: the SETTINGS rules alone; MX_ERR_INVALID names the rule in mx_last_error. */
int mx_deck_analysis_check(const mx_deck_analysis* a);
/* Host only: TABLES.  Sets a->taps and fills a->lo / a->hi (entries from `taps` on 0); column, max_lag and _pad are left alone.  rate not finite and positive, cutoffs
 * not 0 < f_lo < f_hi < rate / 2, taps even or outside 1 .. 127, or tables whose sum |c| exceeds 32767 (cutoffs close to rate / 2): MX_ERR_INVALID, *a untouched. */
int mx_deck_analysis_bands(double rate, double f_lo, double f_hi, uint32_t taps, mx_deck_analysis* a);
/* Analyse the whole track as loaded now.  Asynchronous, on the deck's own load stream: ordered after earlier mx_deck_load_i16 calls and before later ones; it uses
 * neither a graph's stream nor the host, and feeds are not ordered against it (both only read the track).  The results live in device memory the deck owns,
 * N * 56 + N * 4 + L * 8 bytes; a later analysis replaces them, NULL frees them.  The result is a snapshot: a later load does not invalidate it.  Settings that fail the
 * check: MX_ERR_INVALID, and the deck keeps what it had.  Memory that cannot be had: MX_ERR_NOMEM, and the deck is left without an analysis. */
int mx_deck_analyse(mx_deck* d, const mx_deck_analysis* a);
/* Host only: *n = ceil(n_frames / column).  n_frames outside 1 .. 2^30 or a column the check refuses: MX_ERR_INVALID. */
int mx_deck_column_count(uint64_t n_frames, uint32_t column, uint64_t* n);
/* Columns [first, first + n) of the deck's analysis; waits for it (as mx_deck_read_grains waits for a feed).  No analysis, or a window beyond N: MX_ERR_INVALID. */
int mx_deck_read_columns(mx_deck* d, uint64_t first, uint64_t n, mx_deck_column* dst);
/* R[0 .. L) of the deck's analysis into R[0 .. cap); waits for it.  No analysis, or cap below L: MX_ERR_INVALID. */
int mx_deck_read_autocorr(mx_deck* d, uint64_t* R, uint32_t cap);
/* Host only, pure: COLUMNS and ONSET in plain C++ for columns [first, first + n) of a track of n_frames interleaved stereo frames (1 .. 2^30) -- how the rules are
 * tested without a device, and the single-thread baseline of the device path.  R_or_null not NULL: AUTOCORR too, into R_or_null[0 .. max_lag); that needs all the
 * columns, first = 0 and n = N.  Settings the check refuses, a window beyond N, R_or_null with another window, a NULL pointer: MX_ERR_INVALID. */
int mx_deck_columns_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_analysis* a, uint64_t first, uint64_t n, mx_deck_column* cols, uint64_t* R_or_null);
/* Host only, pure: BEAT GRID from n_cols columns and R[0 .. max_lag).  column / max_lag outside the SETTINGS rules, rate, bpm_lo, bpm_hi not finite and positive or
 * bpm_lo > bpm_hi, a NULL pointer (cols may be NULL when n_cols is 0): MX_ERR_INVALID. */
int mx_deck_beatgrid(const mx_deck_column* cols, uint64_t n_cols, const uint64_t* R, uint32_t max_lag, uint32_t column, double rate, double bpm_lo, double bpm_hi,
                     mx_deck_grid* out);
/* DEBUG: what the last mx_deck_analyse of this process launched for the columns: out[0] workgroups that each covered several columns (C < 1024), out[1] workgroups
 * that each took one column in several tiles of 1024 frames (C > 1024), out[2] 1 when the track was shorter than the halo (n_frames < K - 1: one workgroup, a lane
 * per frame), out[3] workgroups of one column in one tile (C = 1024).  Tests use it to know every form ran. */
int mx_deck_debug_last_analysis(uint32_t out[4]);

/* ---- KEY AND LOUDNESS: the whole track's constant-Q sums and its K-weighted loudness, before it sounds ----
 * BUILD-SPECIFIED.  Two more analyses of the track as it lies in device memory, each asynchronous on the deck's own load stream like mx_deck_analyse: ordered after
 * earlier mx_deck_load_i16 calls and before later ones, not ordered against feeds (both only read the track).  Each keeps its results in device memory the deck owns; a
 * later call of the same kind replaces them, NULL frees them; a result is a snapshot that a later load does not invalidate.  The two are independent of each other and
 * of mx_deck_analyse's results.  No arithmetic rule is new: the tonality taps' and the loudness taps' texts above hold word for word, read over one stream that is the
 * track.  A deck that never calls them is untouched in every respect.
 *
 * TONALITY
 * SETTINGS   mx_deck_tonality: decim D, hop_frames Hc, octaves O and f_lo_mhz under the tonality taps' rules (D 4 or 8; Hc 128, 256 or 512; O 2 .. 6; f_lo_mhz >= 1),
 *            and the kernels must exist at `rate` as mx_tonality_tables says (it refuses N_0 > 2048 and a top bin at 0.45 fs_d); segment_hops G 1 .. 65536; rate finite
 *            and positive; _pad 0.  mx_deck_tonality_check enforces exactly these rules.
 * STREAM     F = G Hc D frames make a segment, n_seg = ceil(n_frames / F).  The stream is frames 0 .. n_seg F - 1 of the track; frames at or beyond n_frames read as 0
 *            (the deck's own rule).  Every hop of that stream counts, so every segment has G hops.
 * QUANTISE   s[f] = L[f] + R[f] of the raw int16 (key-lock's and ANALYSIS' s); q[f] = s[f] / 4 with C's integer division, which truncates toward zero.  That IS the
 *            tap's q for L = l / 32768, R = r / 32768: m = (l + r) / 32768 is exact in f32, |m| <= 2, and trunc(m 8192) = trunc(s / 4).  It is not s >> 2 (they differ
 *            for a negative s that is no multiple of 4).  nonfinite is always 0.
 * DECIMATE, KERNELS, HOP   the tonality taps' text unchanged, with the tables of mx_tonality_tables(rate, ...): d[n] = (sum_k c[k] q[n D - k]) >> 15,
 *            M_b[h] = isqrt((S_re >> 10)^2 + (S_im >> 10)^2); q and d at negative indices are 0.
 * RECORDS    n_seg records of mx_tonality_record_bytes each, in the tap's own layout (mx_tonality_chroma and mx_tonality_key take them as they are): the header is
 *            { g, G, 0, D, Hc, O, f_lo_mhz, 0 }, and C[b] = the sum of M_b[h] over the hops h of [g G, (g + 1) G).
 * IT FOLLOWS that record g equals byte for byte what a tonality tap with emit_ticks 1 emits for tick g of a run over the zero-padded track, L = l / 32768 and
 *            R = r / 32768, in ticks of F frames: hop h completes in the tick that holds input frame ((h + 1) Hc - 1) D, which lies in [g F, (g + 1) F) exactly for the
 *            hops of segment g (tests/tonality_model.py is held to that).
 *
 * LOUDNESS
 * SETTINGS   mx_deck_loudness: rate as mx_loudness_tables accepts it; block_frames F 64 .. 65536; momentary_blocks M and short_blocks S 1 .. 1024 each; _pad 0.
 *            mx_deck_loudness_check enforces exactly these rules.
 * STREAM     n_blocks = ceil(n_frames / F); block k is frames [k F, (k + 1) F), frames at or beyond n_frames read as +0.0f.  A sample is (float)s / 32768.0f per channel
 *            (exact; the deck's rule).
 * RULE       the loudness taps' text unchanged with "tick" read as "block": the biquads and P = carry of mx_loudness_tables(rate, F); the transposed direct form II walk
 *            with every f64 operation rounded on its own; S_0 = +0.0, S_k+1 = Z_k + P S_k with the rows summed left to right; ksq from 8 partials and the 4-2-1
 *            butterfly; both window sums afresh in ascending block from +0.0, blocks before the first reading +0.0; the true peak through interp with 11 frames of
 *            run-in that read +0.0 before frame 0 and are the track's own from then on.
 * RECORDS    mx_loudness_tick itself, n_blocks of them, with frames = F and channels = 2.
 * IT FOLLOWS that the records equal bit for bit what a loudness tap reads from this deck played at unity from frame 0 into a graph of F frames per tick
 *            (tests/loudness_model.py is held to that).
 *
 * READ-OUTS  mx_deck_loudness_gain: gated integrated loudness, true peak and the gain that reaches a target under a ceiling, from the records.  mx_tonality_camelot: the
 *            wheel position of a key ("8A").  Both host only, pure, f64.
 * Out of scope: key tracked within a track beyond what the segment records allow a host to do; tuning other than A = 440 (move f_lo_mhz); analysis of a range of the
 * track; more than two channels; applying the gain (the host sets it on the strip); any change to how a deck plays or to any tap. */
typedef struct { double rate; uint32_t decim, hop_frames, octaves, f_lo_mhz; uint32_t segment_hops; uint32_t _pad; } mx_deck_tonality;   /* 32 bytes */
typedef struct { double rate; uint32_t block_frames, momentary_blocks, short_blocks, _pad; } mx_deck_loudness;   /* 24 bytes */
/* Host only: the TONALITY SETTINGS rules alone; MX_ERR_INVALID names the rule in mx_last_error. */
int mx_deck_tonality_check(const mx_deck_tonality* t);
/* Host only: *n_seg = ceil(n_frames / (G Hc D)).  n_frames outside 1 .. 2^30, settings the check refuses, NULL: MX_ERR_INVALID. */
int mx_deck_tonality_count(uint64_t n_frames, const mx_deck_tonality* t, uint64_t* n_seg);
/* Analyse the whole track's tonality as loaded now (above).  Device memory: n_seg records, n_seg G Hc int16 of decimated frames, and one table set.  Settings that fail the
 * check: MX_ERR_INVALID, and the deck keeps what it had.  Memory that cannot be had: MX_ERR_NOMEM, and the deck is left without this analysis.  NULL frees it. */
int mx_deck_analyse_tonality(mx_deck* d, const mx_deck_tonality* t);
/* Records [first, first + n) into dst[0 .. cap_bytes); waits for the analysis, like mx_deck_read_columns.  No analysis, a window beyond n_seg, cap_bytes below
 * n x record bytes, NULL: MX_ERR_INVALID. */
int mx_deck_read_tonality(mx_deck* d, uint64_t first, uint64_t n, void* dst, size_t cap_bytes);
/* Host only, pure: the TONALITY rules in plain C++ for segments [first, first + n) of a track of n_frames interleaved stereo frames (1 .. 2^30), n x record bytes into
 * dst -- how the rules are tested without a device, and the single-thread baseline of the device path.  Settings the check refuses, a window beyond n_seg, NULL:
 * MX_ERR_INVALID. */
int mx_deck_tonality_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_tonality* t, uint64_t first, uint64_t n, void* dst);
/* DEBUG: what the last mx_deck_analyse_tonality of this process launched: out[0] decimator workgroups (256 lanes; 512 decimated frames each from one staged window of
 * quantised frames), out[1] constant-Q workgroups that took a full 8 hops of a segment (256 lanes: 8 hops staged at once, a wave per bin, every table entry loaded once
 * for the 8), out[2] constant-Q workgroups that took fewer (the tail of a segment, or G < 8), out[3] workgroups of the kernel that writes the headers and zeroes the sums
 * (256 lanes, one per 64-bit word).  Tests use it to know every form ran. */
int mx_deck_debug_last_tonality(uint32_t out[4]);
/* Host only: the LOUDNESS SETTINGS rules alone; MX_ERR_INVALID names the rule in mx_last_error. */
int mx_deck_loudness_check(const mx_deck_loudness* l);
/* Host only: *n_blocks = ceil(n_frames / block_frames).  n_frames outside 1 .. 2^30, block_frames outside 64 .. 65536, NULL: MX_ERR_INVALID. */
int mx_deck_loudness_count(uint64_t n_frames, uint32_t block_frames, uint64_t* n_blocks);
/* Analyse the whole track's loudness as loaded now (above).  Device memory: n_blocks x (48 bytes of records + 64 bytes of walk states).  Refusals as
 * mx_deck_analyse_tonality; NULL frees it. */
int mx_deck_analyse_loudness(mx_deck* d, const mx_deck_loudness* l);
/* Records [first, first + n); waits for the analysis.  No analysis, a window beyond n_blocks, NULL: MX_ERR_INVALID. */
int mx_deck_read_loudness(mx_deck* d, uint64_t first, uint64_t n, mx_loudness_tick* dst);
/* Host only, pure: the LOUDNESS rules in plain C++ for the whole track (the state is a recurrence: there is no window), n_blocks records into dst[0 .. cap).  Settings
 * the check refuses, n_frames outside 1 .. 2^30, cap below n_blocks, NULL: MX_ERR_INVALID. */
int mx_deck_loudness_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_loudness* l, mx_loudness_tick* dst, uint64_t cap);
/* DEBUG: what the last mx_deck_analyse_loudness of this process launched: out[0] true-peak workgroups (256 lanes; a tile of 1024 frames staged once with its 11-frame
 * run-in, a lane per frame), out[1] walk workgroups of EACH of the two walks (one wave; 32 blocks, a lane per block and channel), out[2] steps of the one serial scan
 * (n_blocks; one lane per channel), out[3] window workgroups (256 lanes, one per block).  Tests use it to know every form ran. */
int mx_deck_debug_last_loudness(uint32_t out[4]);
/* Host only, pure, f64: programme loudness, true peak and gain from n records of one analysis (or one tap).  The measurement blocks are the records
 * i = i0, i0 + hop_blocks, ... < n with i0 = min(momentary_blocks - 1, n - 1); each has block_sq = recs[i].momentary_sq over momentary_blocks x recs[i].frames frames.
 * *lufs = what mx_loudness_gate says of them (-inf when nothing passes the gates); *peak_dbtp = 20 log10 of the largest true_peak over all records and both channels,
 * -inf for 0; *gain_db = min(target_lufs - *lufs, ceiling_dbtp - *peak_dbtp), and 0 when *lufs is -inf.  With F = 4800 at 48 kHz, momentary_blocks = 4 and
 * hop_blocks = 1 the blocks are the standard's 400 ms at 75 % overlap.  n = 0, hop_blocks = 0, momentary_blocks outside 1 .. 1024, a record of 0 frames, NULL, a target or
 * ceiling that is not finite: MX_ERR_INVALID. */
int mx_deck_loudness_gain(const mx_loudness_tick* recs, uint64_t n, uint32_t momentary_blocks, uint32_t hop_blocks, double target_lufs, double ceiling_dbtp,
                          double* lufs, double* peak_dbtp, double* gain_db);
/* Host only: the Camelot wheel position DJs read for a key of mx_tonality_key.  With t the tonic: major (key 0 .. 11, t = key): *number = ((7 t + 7) mod 12) + 1,
 * *minor = 0 ("B"); minor (key 12 .. 23, t = key - 12): *number = ((7 t + 4) mod 12) + 1, *minor = 1 ("A").  C major is 8B, A minor 8A, B major 1B.  A key outside
 * 0 .. 23 (-1 included) or NULL: MX_ERR_INVALID. */
int mx_tonality_camelot(int key, uint32_t* number, uint32_t* minor);

/* ---- FINE GRID: the beat period and phase of a whole track to a fine hop, by a comb search on the device, and the arithmetic that puts two decks in time ----
 * BUILD-SPECIFIED.  mx_deck_beatgrid reads a tempo: its period comes from a parabola through three lags of columns (good to about 1e-3 of a beat, which over the 1 200
 * beats of a ten-minute track is more than a beat) and its phase is good to a column.  This section turns that read-out into a grid: around a coarse period it tries
 * up to 8192 candidate periods, each at every integer phase, and scores each by the onset weight a comb of that period and phase collects over the track.  A fourth
 * analysis on the deck's own load stream, with the ownership rules of the other three and independent of their results; integers throughout, so the records are fixed
 * count for count.  A deck that never calls it is untouched in every respect, and mx_deck_analyse / mx_deck_beatgrid / mx_deck_grid are what they were.
 *
 * SETTINGS   mx_deck_finegrid: hop h a power of two, 16 .. 256 frames; n_periods 1 .. 8192; candidate j has the period P_j = period0_q16 + j * dperiod_q16 in fine hops,
 *            Q16, and every P_j lies in [4 * 65536, 32768 * 65536]; dperiod_q16 >= 1 unless n_periods is 1; first_hop < N; max_beats 0 (all teeth) or >= 2; _pad 0.
 *            mx_deck_finegrid_check enforces exactly these rules for a track of n_frames (1 .. 2^30).
 * ONSETS     N = ceil(n_frames / h).  s[f] = L[f] + R[f] of the raw int16 track (ANALYSIS' and key-lock's s).  e[i] = the sum of s[f]^2 over the frames f of
 *            [i h, (i + 1) h) with f < n_frames (at most 2^40); A[i] = floor(sqrt(e[i])), the exact integer root, A[-1] = 0; o[i] = max(A[i] - A[i - 1], 0) >> 4
 *            (subtract, clamp, then shift; at most 2^16).  The tooth weight is w[i] = o[i - 1] + 2 o[i] + o[i + 1] with o read as 0 outside [0, N) (at most 2^18):
 *            a tooth three hops wide and centre-weighted, so that a comb with an integer phase and a fractional period can sit on every beat of a track whose beats
 *            do not fall on hops.
 * COMB       for candidate j and each integer phase phi, 0 <= phi < ceil(P_j) = (P_j + 65535) >> 16:
 *                S(j, phi) = sum over k = 0, 1, ... of w[i_k],    i_k = first_hop + phi + ((k * P_j) >> 16)
 *            the sum stopping at the first k with i_k >= N, or at k = max_beats when that is not 0.  64-bit integers: k * P_j < 2^57, S < 2^44.  The record of
 *            candidate j, mx_deck_comb (16 bytes): score the largest S, phase the smallest phi that reaches it, beats the number of teeth that phase summed (0 when
 *            its first tooth already lies beyond the track).
 * PICK       mx_deck_finegrid_pick, host only and pure: the largest score, then the smallest j.  mx_deck_beats in track frames, Q32.32:
 *            period_q32 = (P_j * h) << 16, first_q32 = ((first_hop + phase) * h + h / 2) << 32 -- the centre of tooth 0; beat n lies at first_q32 + n * period_q32.
 *            mx_deck_fine_pick adds index j, score, n_beats = beats and bpm = (60.0 * rate * 65536.0) / ((double)P_j * (double)h), every f64 operation separate and left
 *            to right.  With every score 0 the result is all zero.
 * SPAN       mx_deck_finegrid_span, host only and pure, fills the settings of one stage of a search from a centre period c and a half-width (both Q16 hops), a beat
 *            limit B (0: the whole track), N and h.  K = ceil(N * 65536 / c), the teeth of phase 0 that fit, or B if B is not 0 and smaller; dperiod = max(1,
 *            floor(32768 / K)), so neighbouring candidates move the last tooth by at most half a hop; m = min(ceil(half-width / dperiod), 4095), further cut on either
 *            side to what stays within [4 * 65536, 32768 * 65536]; n_periods = m_below + m_above + 1 with c itself a candidate; first_hop 0, max_beats B.
 *            *clipped says whether any cut was made.  Two stages reach the whole track's precision: stage one from the coarse period c with a half-width of
 *            ceil(c / 50) (+-2 %) and B = 64, stage two from stage one's winner with a half-width of 4 x stage one's dperiod and B = 0.  (Four, not one: a tooth
 *            reaches 1.5 hops to either side of its centre and the beat itself is quantised to a hop, so every candidate whose LAST tooth of stage one lies within 2
 *            hops of the true one can collect the same onsets and win; neighbours move that tooth by at most half a hop, which makes 4 steps.)
 *            mx_deck_finegrid_period converts mx_deck_grid.period_columns: the integer nearest to period_columns * C / h * 65536 (C / h a power of two: one
 *            rounding, ties to even).
 * SYNC       mx_deck_sync, host only, pure, exact (128-bit integers, as mx_deck_step): from the leader's beats, position and step and the follower's beats and
 *            position, all as of the start of the same tick, the follower's step and the position it must stand at so that its beats fall on the leader's.  With Pl,
 *            Pf the two periods, every division rounded to nearest, ties to even:
 *                step  = sign(leader_step) * round(|leader_step| * Pf / Pl)                              (|step| > 4 * 2^32: MX_ERR_INVALID)
 *                a     = floor_mod(leader_pos - first_l, Pl),   b = round(a * Pf / Pl),   c = floor_mod(follower_pos - first_f, Pf)
 *                delta = b - c, then Pf added or subtracted until it lies in (-Pf / 2, Pf / 2],   seek = follower_pos + delta
 *            The host hands step and seek to mx_deck_schedule for that tick.  A period outside [1, 2^56], a position or first beat beyond 2^62 in magnitude: MX_ERR_INVALID.
 * Out of scope: a key-locked leader or follower (under KEY-LOCK the head still crosses the track as mx_deck_plan says, so the arithmetic holds for the head; what the
 * grains make audible of it is KEY-LOCK's business, and nothing here refuses such a deck); tempo that changes within a track (TEMPO MAP below); downbeats and bars (BARS below); phases finer than a
 * hop; a search over a range of the track other than "from first_hop on". */
#define MX_DECK_FINEGRID_LANES 256u       /* phases one pass of a comb workgroup covers (a lane per phase); tests size their candidates around it */
#define MX_DECK_FINEGRID_MAX_PERIODS 8192u
typedef struct { uint32_t hop; uint32_t n_periods; uint64_t period0_q16; uint32_t dperiod_q16; uint32_t first_hop; uint32_t max_beats; uint32_t _pad; } mx_deck_finegrid;   /* 32 bytes */
typedef struct { uint64_t score; uint32_t phase; uint32_t beats; } mx_deck_comb;   /* 16 bytes */
typedef struct { int64_t first_q32; int64_t period_q32; } mx_deck_beats;
typedef struct { mx_deck_beats grid; uint64_t score; double bpm; uint32_t index; uint32_t n_beats; } mx_deck_fine_pick;   /* 40 bytes */
typedef struct { int64_t step_q32; int64_t seek_q32; int64_t delta_q32; } mx_deck_sync_result;
/* Host only: the SETTINGS rules alone for a track of n_frames; MX_ERR_INVALID names the rule in mx_last_error. */
int mx_deck_finegrid_check(const mx_deck_finegrid* s, uint64_t n_frames);
/* Host only: *n_hops = N = ceil(n_frames / hop).  n_frames outside 1 .. 2^30 or a hop the check refuses: MX_ERR_INVALID. */
int mx_deck_finegrid_count(uint64_t n_frames, uint32_t hop, uint64_t* n_hops);
/* Host only, pure: SPAN.  centre_q16 outside [4 * 65536, 32768 * 65536], n_hops outside 1 .. 2^26, a hop the check refuses, beat_limit 1, NULL (clipped may be NULL):
 * MX_ERR_INVALID, *s untouched. */
int mx_deck_finegrid_span(uint64_t centre_q16, uint64_t halfwidth_q16, uint32_t beat_limit, uint64_t n_hops, uint32_t hop, mx_deck_finegrid* s, uint32_t* clipped);
/* Host only: SPAN's conversion of a coarse period.  A value that is not finite, column outside ANALYSIS' rule, a hop the check refuses, a result outside
 * [4 * 65536, 32768 * 65536]: MX_ERR_INVALID. */
int mx_deck_finegrid_period(double period_columns, uint32_t column, uint32_t hop, uint64_t* period_q16);
/* Score every candidate over the whole track as loaded now.  Asynchronous on the deck's own load stream, like mx_deck_analyse: ordered after earlier loads and before
 * later ones, not ordered against feeds.  Device memory the deck owns: 8192 * 16 + N * 4 bytes (room for any n_periods, so a second stage at the same hop never grows
 * the buffer); a later call replaces the result (a buffer that must grow, for a smaller hop, waits for the stream first), NULL frees it; the result is a snapshot that a later load does not invalidate, and each call computes w afresh.  Settings the check refuses:
 * MX_ERR_INVALID, and the deck keeps what it had.  Memory that cannot be had: MX_ERR_NOMEM, and the deck is left without a fine grid. */
int mx_deck_analyse_finegrid(mx_deck* d, const mx_deck_finegrid* s);
/* Records [first, first + n) of the deck's fine grid; waits for it, like mx_deck_read_columns.  No fine grid, a window beyond n_periods, NULL: MX_ERR_INVALID. */
int mx_deck_read_finegrid(mx_deck* d, uint64_t first, uint64_t n, mx_deck_comb* dst);
/* w[first .. first + n) of the deck's fine grid; waits for it.  No fine grid, a window beyond N, NULL: MX_ERR_INVALID. */
int mx_deck_read_fine_onsets(mx_deck* d, uint64_t first, uint64_t n, uint32_t* w);
/* Host only, pure: ONSETS and COMB in plain C++ over a track of n_frames interleaved stereo frames: n_periods records into recs, and w[0 .. N) into w_or_null when it is
 * not NULL -- how the rules are tested without a device, and the single-thread baseline of the device path.  Settings the check refuses, NULL: MX_ERR_INVALID. */
int mx_deck_finegrid_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_finegrid* s, mx_deck_comb* recs, uint32_t* w_or_null);
/* Host only, pure: PICK from the n_periods records of settings s.  s outside the SETTINGS rules (first_hop is not held against a track), rate not finite and positive,
 * NULL: MX_ERR_INVALID. */
int mx_deck_finegrid_pick(const mx_deck_comb* recs, const mx_deck_finegrid* s, double rate, mx_deck_fine_pick* out);
/* Host only, pure, exact: SYNC. */
int mx_deck_sync(const mx_deck_beats* leader, int64_t leader_pos_q32, int64_t leader_step_q32, const mx_deck_beats* follower, int64_t follower_pos_q32,
                 mx_deck_sync_result* out);
/* Host only, pure, exact (ECHO above): *delay = the integer nearest to period_q32 * num / (|step_q32| * den), the output frames of num / den beats of `grid` at this
 * step, in 128-bit integers with ties to even: 3/4 beat of 126.4 BPM at 48 kHz and unity is 17 089.  step, num or den 0, a grid without a positive period, a result
 * outside MX_DECK_ECHO_MIN_DELAY .. MX_DECK_ECHO_MAX_DELAY, NULL: MX_ERR_INVALID. */
int mx_deck_echo_delay(const mx_deck_beats* grid, int64_t step_q32, uint32_t num, uint32_t den, uint32_t* delay);
/* DEBUG: what the last mx_deck_analyse_finegrid of this process launched: out[0] comb workgroups (one per candidate, MX_DECK_FINEGRID_LANES lanes) whose phases fit one
 * pass of the lanes, out[1] comb workgroups that looped over the phases in strides, out[2] onset workgroups (256 lanes; 256 hops of w each), out[3] the trip count of
 * the comb kernel's loop over k (the teeth of phase 0 at the smallest period, or max_beats).  Tests use it to know every form ran. */
int mx_deck_debug_last_finegrid(uint32_t out[4]);

/* ---- BARS: downbeats and phrase lines of a whole track from the novelty of its beats, on the device ----
 * BUILD-SPECIFIED.  The fine grid knows every beat and nothing above a beat.  This section finds which beat is a bar's first and which bar a phrase's first, by the rule
 * "arrangements change on bar lines, and most of all on phrase lines": per beat of a given grid a small band-energy vector, a checkerboard novelty over the beats'
 * pairwise distances at a bar-sized and at a phrase-sized width, and both novelties folded by beat index modulo the bar and modulo the phrase.  A fifth analysis on the
 * deck's own load stream with the ownership rules of the other four and independent of their results; integers throughout, so the records are fixed count for count.
 * A deck that never calls it is untouched in every respect, and mx_deck_analyse*, mx_deck_sync and mx_deck_echo_delay are what they were.
 *
 * SETTINGS   mx_deck_bars: grid the beats (FINE GRID's mx_deck_beats), period_q32 in [2048 * 2^32, 2^17 * 2^32] -- a half-beat is then at least 1024 frames, and a
 *            half-beat's band energy (band^2 <= 2^36 over at most 2^16 frames) stays below 2^53, tempo_root's domain -- and |first_q32| <= 2^62; lead 0 .. 4096
 *            frames; taps K odd, 1 .. 127; beats_per_bar M 2 .. 8; bars_per_phrase Q 1 .. 16; w_bar and w_phrase 1 .. 64 beats; max_beats (0: all); lo[0 .. K) and
 *            hi[0 .. K) under ANALYSIS' rules exactly (Q14, sum |c_k| <= 32767, entries at index K and above 0).  The struct has no hole and no padding field (552
 *            bytes).  mx_deck_bars_tables copies taps, lo and hi from an mx_deck_analysis that mx_deck_analysis_bands filled.  mx_deck_bars_check enforces exactly
 *            these rules for a track of n_frames (1 .. 2^30), and refuses a grid that places no whole beat in the track, and one whose n_beats (BEATS: after
 *            max_beats has cut it) is above MX_DECK_BARS_MAX_BEATS: a longer track is analysed over its first max_beats beats.
 * BEATS      f(j) = ((first_q32 + j * period_q32) >> 32) - lead  (in integers that do not overflow; arithmetic shift: floor).  n0 is the smallest integer j, negative
 *            ones included, with f(j) >= 0.  Beat k >= 0 covers the frames [f(n0 + k), f(n0 + k + 1)).  n_beats is the number of k whose beat ends at or before
 *            n_frames (whole beats only), then cut to max_beats when that is not 0.  mx_deck_bars_count returns n_beats and n0 (host only).  lead is there because
 *            a grid line is the centre of a tooth: the burst's first frames lie up to 1.5 fine hops before it.
 * FEATURES   s, low, mid, high are ANALYSIS' SIGNAL, frame for frame (s zero outside the track, so the filter's halo reads zeros there).  With a, c the beat's ends
 *            and h = a + ((c - a) >> 1), the beat's vector is v[0 .. 3) = floor(sqrt(sum band^2)) over the frames of [a, h) for low, mid, high -- the exact integer
 *            root, tempo_root -- and v[3 .. 6) the same over [h, c).  d(i, j) = sum over the six components of |v[i][c] - v[j][c]| (below 2^30).
 * NOVELTY    for a width W and W <= k <= n_beats - W, with P = [k - W, k) and F = [k, k + W):
 *                N_W[k] = 2 sum_{a in P, b in F} d(a, b) - sum_{a, a' in P} d(a, a') - sum_{b, b' in F} d(b, b')
 *            the two last sums over ORDERED pairs (each unordered pair twice; d(a, a) = 0).  N_W[k] = 0 for every other k.  The type is int64 and |N| < 2^44.  N is
 *            never negative: per component it is W^2 times the energy distance of the two halves' values, 2 W^2 times the integral of (F_P - F_F)^2 over their
 *            empirical distribution functions.  FOLD's clamp therefore changes nothing on the records of an analysis; it stays in the rule for a host that folds
 *            novelties of its own making.
 *            The record of beat k, mx_deck_beat (48 bytes): v[6], first_frame = f(n0 + k), frames = the beat's length, n_bar = N at W = w_bar, n_phrase = N at
 *            W = w_phrase.
 * FOLD       H_bar[m] = sum over k = m (mod M) of max(n_bar[k], 0) for m < M; H_phrase[m] = sum over k = m (mod M Q) of max(n_phrase[k], 0) for m < M Q: the clamp
 *            per beat, before the sum.  uint64, M + M Q words (136 at the most), H_bar first; in device memory they lie behind the room for the records.
 * PICK       mx_deck_bars_pick, host only, pure and exact.  The bar phase mb is the smallest m of the largest H_bar; the phrase phase mp is, among the m = mb (mod M),
 *            the smallest of the largest H_phrase.  mx_deck_bar_pick (72 bytes): bars = { first_q32 + (n0 + mb) * period_q32, M * period_q32 }; phrases the same
 *            with mp and M Q (at most 2^56, mx_deck_sync's bound); bar_phase = mb, phrase_phase = mp; bar_best = H_bar[mb], bar_sum = sum of H_bar,
 *            phrase_best = H_phrase[mp], phrase_sum = the sum of H_phrase over the m = mb (mod M).  Confidence is best / sum, left to the caller.  With
 *            bar_sum = 0 everything is zero.  Bar-aligned sync is mx_deck_sync on two `bars` grids.
 * NEXT LINE  mx_deck_grid_next, host only, pure and exact (128-bit integers): the smallest n with first_q32 + n * period_q32 >= pos_q32 -- n = ceil((pos - first) /
 *            period) by floor division, negative positions and indices included -- and that line.  On a beat, bar or phrase grid: what a host needs to schedule an
 *            echo-out or a loop on the coming line.  mx_deck_sync's range rules: a period outside [1, 2^56], a position or first beat beyond 2^62 in magnitude:
 *            MX_ERR_INVALID (|n| then stays below 2^63 but for pos = 2^62, first = -2^62, period = 1, which is refused too).
 * Out of scope: metre detection (M is given); tempo that changes within a track; section labels and thresholds on phrase lines; chroma in the vector; analysis of a
 * range of the track; any change to sync itself. */
#define MX_DECK_BARS_MAX_BEATS 16384u
#define MX_DECK_BARS_MAX_FOLDS 136u     /* M + M Q at M = 8, Q = 16 */
#define MX_DECK_BARS_BLOCK 4u           /* beats one novelty workgroup takes (a wave per beat); tests size their cases around it */
typedef struct { mx_deck_beats grid; uint32_t lead; uint32_t taps; uint32_t beats_per_bar; uint32_t bars_per_phrase; uint32_t w_bar; uint32_t w_phrase; uint32_t max_beats;
                 int16_t lo[127]; int16_t hi[127]; } mx_deck_bars;   /* 552 bytes */
typedef struct { uint32_t v[6]; uint32_t first_frame; uint32_t frames; int64_t n_bar; int64_t n_phrase; } mx_deck_beat;   /* 48 bytes */
typedef struct { mx_deck_beats bars; mx_deck_beats phrases; uint32_t bar_phase; uint32_t phrase_phase; uint64_t bar_best; uint64_t bar_sum; uint64_t phrase_best;
                 uint64_t phrase_sum; } mx_deck_bar_pick;   /* 72 bytes */
/* Host only: the SETTINGS rules alone for a track of n_frames; MX_ERR_INVALID names the rule in mx_last_error. */
int mx_deck_bars_check(const mx_deck_bars* s, uint64_t n_frames);
/* Host only: BEATS.  *n_beats and *n0 (either may be NULL) of settings the check accepts; otherwise MX_ERR_INVALID. */
int mx_deck_bars_count(const mx_deck_bars* s, uint64_t n_frames, uint32_t* n_beats, int64_t* n0);
/* Host only: copies taps, lo and hi of *a (which must pass mx_deck_analysis_check) into *s and leaves the rest of *s alone.  Otherwise MX_ERR_INVALID, *s untouched. */
int mx_deck_bars_tables(const mx_deck_analysis* a, mx_deck_bars* s);
/* Analyse the whole track as loaded now.  Asynchronous on the deck's own load stream, like mx_deck_analyse: ordered after earlier loads and before later ones, not
 * ordered against feeds.  Device memory the deck owns: 16384 * 48 + 136 * 8 bytes whatever the settings, so no later call grows it; a later call replaces the result,
 * NULL frees it; the result is a snapshot that a later load does not invalidate.  Settings the check refuses: MX_ERR_INVALID, and the deck keeps what it had.  Memory
 * that cannot be had: MX_ERR_NOMEM, and the deck is left without this analysis. */
int mx_deck_analyse_bars(mx_deck* d, const mx_deck_bars* s);
/* Records [first, first + n) of the deck's bars analysis; waits for it, like mx_deck_read_columns.  No analysis, a window beyond n_beats, NULL: MX_ERR_INVALID. */
int mx_deck_read_bars(mx_deck* d, uint64_t first, uint64_t n, mx_deck_beat* dst);
/* H_bar[0 .. M) and then H_phrase[0 .. M Q) of the deck's bars analysis into H[0 .. cap); waits for it.  No analysis, cap below M + M Q, NULL: MX_ERR_INVALID. */
int mx_deck_read_bar_folds(mx_deck* d, uint64_t* H, uint32_t cap);
/* Host only, pure: BEATS, FEATURES, NOVELTY and FOLD in plain C++ over a track of n_frames interleaved stereo frames: n_beats records into recs and M + M Q words into
 * H_or_null when it is not NULL -- how the rules are tested without a device, and the single-thread baseline of the device path.  Settings the check refuses, NULL:
 * MX_ERR_INVALID. */
int mx_deck_bars_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_bars* s, mx_deck_beat* recs, uint64_t* H_or_null);
/* Host only, pure, exact: PICK from the M + M Q words H of settings s.  Every SETTINGS rule that needs no track is held (not the two about the beats a grid places);
 * otherwise, or with NULL: MX_ERR_INVALID. */
int mx_deck_bars_pick(const uint64_t* H, const mx_deck_bars* s, mx_deck_bar_pick* out);
/* Host only, pure, exact: NEXT LINE.  index or line_q32 may be NULL. */
int mx_deck_grid_next(const mx_deck_beats* grid, int64_t pos_q32, int64_t* index, int64_t* line_q32);
/* DEBUG: what the last mx_deck_analyse_bars of this process launched: out[0] band-pass workgroups (one per half-beat, 256 lanes) whose half-beat fits one tile of 1024
 * frames, out[1] those that walked several tiles, out[2] novelty workgroups (MX_DECK_BARS_BLOCK beats each, a wave per beat), out[3] the novelties (a beat at a width)
 * that NOVELTY defines and a wave summed, the others being written as 0.  Tests use it to know every form ran. */
int mx_deck_debug_last_bars(uint32_t out[4]);

/* ---- TEMPO MAP: the beats of a track whose tempo drifts, by a comb search per window of the track on the device, and the arithmetic that follows the map ----
 * BUILD-SPECIFIED.  FINE GRID fits one period and one phase to a whole track; a live drummer, a record cut before sequencers or a single tempo change leaves such a
 * grid half a beat off at the track's ends.  This section runs FINE GRID's comb inside overlapping windows of the track, every candidate period at every integer phase
 * in every window; the host then picks one candidate per window by a path that pays for tempo jumps, turns the picks into segments that each carry an ordinary
 * mx_deck_beats, and looks the segment of a position up -- whose grid goes into mx_deck_sync, mx_deck_echo_delay and mx_deck_grid_next unchanged.  A sixth analysis on
 * the deck's own load stream with the ownership rules of the other five and independent of their results (the fine grid's included); integers throughout, so the
 * records are fixed count for count.  A deck that never calls it is untouched in every respect, and every other entry point is what it was.
 *
 * SETTINGS   mx_deck_tempomap (32 bytes): hop h and the candidate periods P_j = period0_q16 + j * dperiod_q16 under FINE GRID's rules (h a power of two, 16 .. 256;
 *            every P_j in [4 * 65536, 32768 * 65536]; dperiod_q16 >= 1 unless n_periods is 1), with n_periods 1 .. MX_DECK_TEMPOMAP_MAX_PERIODS; window_hops W with
 *            2 * ceil(P_max) <= W <= MX_DECK_TEMPOMAP_MAX_WINDOW (P_max the largest candidate, ceil(P) = (P + 65535) >> 16: every phase of every candidate has a
 *            second tooth's room in a full window, and a window's w is at most 64 KB); stride_hops T with 1 <= T <= W; _pad 0.  For a track of n_frames
 *            (1 .. 2^30), N = ceil(n_frames / h) and the window count is V = 1 when N <= W, else ceil((N - W) / T) + 1; V * n_periods <= 2^20.
 *            mx_deck_tempomap_check enforces exactly these rules, in this order, and names the broken one; mx_deck_tempomap_count returns V.
 * ONSETS     w[i], 0 <= i < N, is FINE GRID's tooth weight over the whole track, number for number.
 * COMB       window v covers the hops [v T, E_v), E_v = min(v T + W, N); the last window ends at N and is never empty.  For candidate j and each integer phase phi,
 *            0 <= phi < ceil(P_j):
 *                S_v(j, phi) = sum over k = 0, 1, ... of w[i_k],    i_k = v T + phi + ((k * P_j) >> 16)
 *            the sum stopping at the first k with i_k >= E_v.  Record (v, j), an mx_deck_comb at index v * n_periods + j: score the largest S, phase the smallest
 *            phi that reaches it, beats the number of teeth that phase summed.  A phase whose first tooth lies at or beyond E_v (a last window shorter than
 *            ceil(P_j)) has S = 0 and 0 teeth.  With W >= N there is one window, and its records are FINE GRID's at first_hop = 0, max_beats = 0, byte for byte.
 *            A score is below 2^30 (w <= 2^18, at most W / 4 = 2^12 teeth).
 * PATH       mx_deck_tempomap_path, host only, pure and exact: one candidate index per window.  With score[v][j] the records' scores,
 *                D[0][j] = score[0][j],    D[v][j] = score[v][j] + max over i of (D[v - 1][i] - penalty * |j - i|),    ties to the smallest i;
 *            the path ends at the largest D[V - 1][j], ties to the smallest j, and is read backwards from there.  penalty is at most 2^40 and every score at most
 *            2^40 (otherwise MX_ERR_INVALID), so with V * n_periods <= 2^20 nothing leaves int64.  penalty 0 is the per-window pick: the largest score of each
 *            window, then the smallest j.
 * SEGMENTS   mx_deck_tempomap_segments, host only, pure and exact: one mx_deck_tempo_segment (40 bytes) per window from the records, the settings and a path.
 *            Window v's own grid, with j the path's index and phase the record's: period_q32 = (P_j * h) << 16, first_q32 = ((v T + phase) * h + h / 2) << 32 --
 *            PICK's, with the window's first hop for first_hop.  score is the record's, window is v.  A window whose chosen score is 0 is a breakdown: its flags
 *            carry MX_DECK_TEMPO_EMPTY and its grid is that of the nearest earlier window that is not empty; empty windows before the first that is not take the
 *            grid of that one; when every window is empty every grid is { 0, 0 }.  start_q32 of segment 0 is -2^62.  For v >= 1 it is the first line of segment
 *            v's grid (the inherited one for an empty window) at or after the position m_v = ((v T + (W - T) / 2) * h) << 32 -- (W - T) / 2 rounded down: the
 *            middle of the overlap with window v - 1 -- as mx_deck_grid_next finds it; with a grid of { 0, 0 } it is m_v itself.  The beats of the map are, per
 *            segment v, the lines b of its grid with start_v <= b and b + period_v / 2 <= start_(v+1) (period / 2 rounded down; no upper bound in the last
 *            segment): the half-period rule keeps a seam from holding two beats a hop apart.  Starts are not forced to ascend (with T far below a period two
 *            neighbours' first lines may cross); LOOK-UP is defined so that this does not matter.
 * LOOK-UP    mx_deck_tempomap_at, host only, pure: the segment of a position is the one with the LARGEST INDEX among those with start_q32 <= pos_q32; *grid is its
 *            grid and *segment its index (either may be NULL).  The grid goes into mx_deck_sync, mx_deck_echo_delay and mx_deck_grid_next unchanged: asked again
 *            tick by tick it is how a follower tracks a drifting leader.  n = 0, a position below segment 0's start or beyond 2^62, NULL segs: MX_ERR_INVALID.
 * WARP       mx_deck_tempomap_step, host only, pure and exact (128-bit integers, ties to even, as mx_deck_sync): *step_q32 = round(period_q32 * 2^32 /
 *            out_period_q32), the step at which this stretch of the track comes out with a beat every out_period_q32 / 2^32 output frames.  A grid period outside
 *            [1, 2^56], out_period_q32 outside [1, 2^56], a result above 4 * 2^32, NULL: MX_ERR_INVALID.
 * SPAN       mx_deck_tempomap_span, host only and pure: SPAN's arithmetic of FINE GRID with K = window_beats (1 .. 4096), the teeth of one window.  dperiod =
 *            max(1, floor(32768 / K)); m = min(ceil(half-width / dperiod), 511), further cut on either side to what stays within [4 * 65536, 8192 * 65536] -- the
 *            periods that leave room for a window under the cap -- with the centre c itself a candidate (a centre outside that range: MX_ERR_INVALID); W =
 *            ceil(window_beats * P_max / 65536), raised to 2 * ceil(P_max), cut to MX_DECK_TEMPOMAP_MAX_WINDOW; T = max(1, floor(stride_beats * c / 65536)) cut to
 *            W (stride_beats 1 .. 4096).  *clipped says whether m, W (by the cap) or T was cut.  The result is held against mx_deck_tempomap_check's rules for a
 *            track of n_hops hops (1 .. 2^26), so a search too large for V * n_periods <= 2^20 is refused here.
 * Out of scope: bars and phrases over a map (BARS takes one grid); key-locked decks (as under FINE GRID); phases finer than a hop; tempo changes faster than a window
 * can follow; the path search on the device; any change to mx_deck_sync's arithmetic. */
#define MX_DECK_TEMPOMAP_MAX_WINDOW 16384u    /* hops of one window: 64 KB of w, which a workgroup can hold in LDS */
#define MX_DECK_TEMPOMAP_MAX_PERIODS 1024u
#define MX_DECK_TEMPOMAP_MAX_RECORDS 1048576u /* V * n_periods */
#define MX_DECK_TEMPOMAP_GROUP 8u             /* candidates of one window that one comb workgroup walks; tests size their cases around it */
#define MX_DECK_TEMPOMAP_STAGED_MAX 10112u /* the longest window (min(W, N) hops) whose comb workgroups stage it in LDS: four such workgroups fit a CU */
#define MX_DECK_TEMPO_EMPTY 1u                /* mx_deck_tempo_segment.flags: the window's chosen score is 0 and the grid is a neighbour's */
typedef struct { uint32_t hop; uint32_t n_periods; uint64_t period0_q16; uint32_t dperiod_q16; uint32_t window_hops; uint32_t stride_hops; uint32_t _pad; } mx_deck_tempomap;   /* 32 bytes */
typedef struct { int64_t start_q32; mx_deck_beats grid; uint64_t score; uint32_t window; uint32_t flags; } mx_deck_tempo_segment;   /* 40 bytes */
/* Host only: the SETTINGS rules alone for a track of n_frames; MX_ERR_INVALID names the rule in mx_last_error. */
int mx_deck_tempomap_check(const mx_deck_tempomap* s, uint64_t n_frames);
/* Host only: *n_windows = V of settings the check accepts; otherwise MX_ERR_INVALID. */
int mx_deck_tempomap_count(const mx_deck_tempomap* s, uint64_t n_frames, uint32_t* n_windows);
/* Host only, pure: SPAN.  *s untouched on MX_ERR_INVALID; clipped may be NULL. */
int mx_deck_tempomap_span(uint64_t centre_q16, uint64_t halfwidth_q16, uint32_t window_beats, uint32_t stride_beats, uint64_t n_hops, uint32_t hop, mx_deck_tempomap* s,
                          uint32_t* clipped);
/* Host only, pure: ONSETS and COMB in plain C++ over a track of n_frames interleaved stereo frames: V * n_periods records into recs, and w[0 .. N) into w_or_null when it
 * is not NULL -- how the rules are tested without a device, and the single-thread baseline of the device path.  Settings the check refuses, NULL: MX_ERR_INVALID. */
int mx_deck_tempomap_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_tempomap* s, mx_deck_comb* recs, uint32_t* w_or_null);
/* Host only, pure, exact: PATH over n_windows * n_periods records (both at least 1, their product at most 2^20): n_windows indices into index. */
int mx_deck_tempomap_path(const mx_deck_comb* recs, uint32_t n_windows, uint32_t n_periods, uint64_t penalty, uint32_t* index);
/* Host only, pure, exact: SEGMENTS.  V = mx_deck_tempomap_count(s, n_frames) entries of index (each below n_periods) are read and V segments written. */
int mx_deck_tempomap_segments(const mx_deck_comb* recs, const mx_deck_tempomap* s, uint64_t n_frames, const uint32_t* index, mx_deck_tempo_segment* segs);
/* Host only, pure: LOOK-UP. */
int mx_deck_tempomap_at(const mx_deck_tempo_segment* segs, uint32_t n, int64_t pos_q32, mx_deck_beats* grid, uint32_t* segment);
/* Host only, pure, exact: WARP. */
int mx_deck_tempomap_step(const mx_deck_beats* grid, int64_t out_period_q32, int64_t* step_q32);
/* Score every candidate in every window over the whole track as loaded now.  Asynchronous on the deck's own load stream, like mx_deck_analyse: ordered after earlier
 * loads and before later ones, not ordered against feeds.  Device memory the deck owns: V * n_periods * 16 + N * 4 bytes; a later call replaces the result (a buffer
 * that must grow waits for the stream first, one that is large enough stays), NULL frees it; the result is a snapshot that a later load does not invalidate, and each
 * call computes w afresh.  Settings the check refuses: MX_ERR_INVALID, and the deck keeps what it had.  Memory that cannot be had: MX_ERR_NOMEM, and the deck is left
 * without a tempo map. */
int mx_deck_analyse_tempomap(mx_deck* d, const mx_deck_tempomap* s);
/* Records [first, first + n) of the deck's tempo map (record (v, j) at v * n_periods + j); waits for it, like mx_deck_read_columns.  No tempo map, a window beyond
 * V * n_periods, NULL: MX_ERR_INVALID. */
int mx_deck_read_tempomap(mx_deck* d, uint64_t first, uint64_t n, mx_deck_comb* dst);
/* w[first .. first + n) of the deck's tempo map; waits for it.  No tempo map, a window beyond N, NULL: MX_ERR_INVALID. */
int mx_deck_read_tempomap_onsets(mx_deck* d, uint64_t first, uint64_t n, uint32_t* w);
/* DEBUG: what the last mx_deck_analyse_tempomap of this process launched: out[0] comb workgroups (256 lanes, one window and up to MX_DECK_TEMPOMAP_GROUP candidates
 * each) that staged their window's w in LDS, out[1] comb workgroups that read w from memory, out[2] onset workgroups (FINE GRID's), out[3] the trip count of the comb
 * kernel's loop over k (the teeth of phase 0 at the smallest period in a window of min(W, N) hops).  One analysis takes one form: the workgroups stage when n_periods is
 * at least 2 and min(W, N) is at most MX_DECK_TEMPOMAP_STAGED_MAX, and read w from memory otherwise.  Tests use it to know every form ran. */
int mx_deck_debug_last_tempomap(uint32_t out[4]);

/* ---- WAVEFORM: the band overview of ANALYSIS rendered to a picture on the device, with beat lines, markers and ranges ----
 * BUILD-SPECIFIED.  mx_deck_render_waveform reads the deck's column records where they lie and writes, in ONE launch, an ordinary opaque yuv420p mx_dframe: the
 * scrolling waveform or the whole-track overview of a deck, ready for mx_video_multiview, mx_video_place, a VideoMixer or mx_graph_set_video_source.  No record is read
 * back and no picture uploaded.  All quantities are integers.  It is deck-side work like the analyses: no module kind, nothing in a graph; a deck that never calls it
 * is untouched in every respect.
 *
 * SETTINGS   mx_deck_waveform (1416 bytes): w, h even, 2 <= w <= 8192, 4 <= h <= 4320; |first_frame| <= 2^30; frames_per_px (fpp) 1 .. 2^20 with w * fpp <= 2^30;
 *            style MX_WAVE_BANDS or MX_WAVE_ENVELOPE; every gain_q16 0 .. 2^20; n_grids <= 16, n_markers <= 32, n_ranges <= 8.  Grid: period_q32 in [2^32, 2^56],
 *            |first_q32| <= 2^61, from_q32 <= to_q32, inset <= h / 2.  Marker: width 1 .. 16.  Range: from_frame <= to_frame.  Every _pad is 0 (the struct's, every
 *            colour's that is looked at, every range's).  Entries at index n_* and above are not looked at.  mx_deck_waveform_check enforces exactly these rules, in
 *            this order -- the struct's scalars, its five colours, then the grids, the markers and the ranges in entry order -- and names the broken one.
 * COLUMN     C and N the column size and count of the analysis, half = h / 2.  Pixel column x covers the frames [F0, F1) = [first_frame + x fpp, first_frame +
 *            (x + 1) fpp) and the analysis columns c0 = max(0, F0 >> log2 C) .. c1 = min(N - 1, (F1 - 1) >> log2 C), the shifts arithmetic (floor).  c0 > c1: the
 *            pixel column is OUTSIDE the track.  Otherwise P_b = max peak[b], SMAX = max smax, SMIN = min smin over those columns; the short last column of a track
 *            counts as a column (so a pixel column whose F0 lies in [n_frames, N C) is inside).
 * HEIGHTS    BANDS: H_b = min(half, (P_b * gain_q16[b] * half) >> 32) in uint64 (at most 2^31 * 2^20 * 2^12).  With d(y) = half - 1 - y for y < half and y - half
 *            otherwise -- rows half - 1 and half both have d = 0 -- band b covers the pixel when d < H_b.  ENVELOPE: UP = min(half, (max(SMAX, 0) * gain_q16[0] *
 *            half) >> 32), DOWN the same from max(-SMIN, 0); the rows [half - UP, half + DOWN) are covered, in colour band[0].
 * LAYERS     bottom to top, each luma pixel ending with one (Y, U, V): (1) bg; (2) each range in entry order whose [from_frame, to_frame) meets [F0, F1) (an empty
 *            range meets nothing): its colour as the background; (3) inside the track, `line` on the rows with d = 0; (4) the bands low, mid, high in that order,
 *            high on top -- or the envelope; outside the track neither; (5) each grid in entry order: rows [inset, h - inset) of every pixel column that holds one
 *            of its lines; (6) each marker in entry order, full height: the pixel columns [xm - width / 2, xm - width / 2 + width) cut to [0, w), xm = floor((frame -
 *            first_frame) / fpp) -- floor division, not C's truncation -- and width / 2 rounded down.  Grids and markers are drawn outside the track too.
 * GRID LINE  n_frames the deck's track length.  F0' and F1' are F0 and F1 clamped to [0, n_frames] FIRST: with that clamp, |first_q32| <= 2^61 and period_q32 <=
 *            2^56, no Q32 quantity below leaves int64 -- which is what those range rules buy.  A = max(F0' << 32, from_q32), B = min(F1' << 32, to_q32).  The pixel
 *            column holds a line of the grid when A < B and first_q32 + ceil((A - first_q32) / period_q32) * period_q32 < B, the ceil mathematical for either sign:
 *            the lines are first + k period for every integer k inside [from, to).  A beat exactly on a pixel's left edge belongs to that pixel, one on its right
 *            edge to the next; a pixel column wholly before frame 0 or at or beyond n_frames holds no line.
 * PLANES     luma is the pixel's Y.  Chroma sample (cx, cy) is (the sum of the four pixels' U + 2) >> 2, likewise V: a one-pixel line tints its chroma sample by a
 *            quarter, or a half where it spans both rows, and does not vanish at odd x.  *out is a NEW opaque yuv420p frame of w x h carrying one reference; every
 *            byte of its three planes, stride padding included, is written exactly once, and the padding holds what mx_video_multiview leaves in its canvas', which
 *            is what mx_dframe_create leaves: Y 0, chroma 0x80.
 * ORDER      the launch goes on `stream` (NULL: the library's default video stream) and waits ON THE DEVICE for the analysis it reads, through an event recorded
 *            behind that analysis on the load stream: a render never waits for the host and never queues behind a later track upload.  The frame is valid on
 *            `stream` on return, like mx_video_multiview's.  A later mx_deck_analyse -- one that rewrites the records in place, regrows them or frees them -- is
 *            ordered behind the deck's last render through a second event, on the device where the buffer stays and by the load stream's own wait where it goes.
 * Out of scope: dimming the played part; text; anti-aliased lines; zoom finer than the analysis' columns (analyse at C = 64 for detail); rendering from PCM; a graph tap
 * that re-renders per tick (call this once per video frame and hand the frame to the graph as a source); more than 16 grid entries -- tempo-map segments -- a picture. */
#define MX_WAVE_BANDS 0u
#define MX_WAVE_ENVELOPE 1u
#define MX_WAVE_MAX_GRIDS 16u
#define MX_WAVE_MAX_MARKERS 32u
#define MX_WAVE_MAX_RANGES 8u
#define MX_WAVE_STRIP 64u                     /* pixel columns one workgroup renders over the full height; tests size their cases around it */
typedef struct { uint8_t y, u, v, _pad; } mx_wave_colour;
typedef struct { mx_deck_beats grid; int64_t from_q32, to_q32; mx_wave_colour colour; uint32_t inset; } mx_wave_grid;   /* 40 bytes: lines at first + k period inside [from, to) */
typedef struct { int64_t frame; uint32_t width; mx_wave_colour colour; } mx_wave_marker;                                /* 16 bytes: cue, loop point, playhead */
typedef struct { int64_t from_frame, to_frame; mx_wave_colour colour; uint32_t _pad; } mx_wave_range;                   /* 24 bytes: loop region, section */
typedef struct {
    uint32_t w, h;                 /* even; 2 <= w <= 8192, 4 <= h <= 4320 */
    int64_t  first_frame;          /* track frame at the left edge of pixel 0; may be negative; |first_frame| <= 2^30 */
    uint32_t frames_per_px;        /* 1 .. 2^20, and w * frames_per_px <= 2^30 */
    uint32_t style;                /* MX_WAVE_BANDS | MX_WAVE_ENVELOPE */
    uint32_t gain_q16[3];          /* per band (ENVELOPE uses [0]); 0 .. 2^20 */
    mx_wave_colour bg, line, band[3];
    uint32_t n_grids, n_markers, n_ranges;
    uint32_t _pad;
    mx_wave_grid grid[MX_WAVE_MAX_GRIDS]; mx_wave_marker marker[MX_WAVE_MAX_MARKERS]; mx_wave_range range[MX_WAVE_MAX_RANGES];
} mx_deck_waveform;                /* 1416 bytes: first_frame 8, frames_per_px 16, gain_q16 24, bg 36, n_grids 56, grid 72, marker 712, range 1224 */
/* Host only: the SETTINGS rules alone; MX_ERR_INVALID names the rule in mx_last_error. */
int mx_deck_waveform_check(const mx_deck_waveform* p);
/* Host only: *first_frame = (pos_q32 >> 32) - playhead_x * frames_per_px (arithmetic shift), the first_frame that puts the playing position in pixel column playhead_x.
 * frames_per_px outside 1 .. 2^20, playhead_x above 8191, a result beyond +-2^30, NULL: MX_ERR_INVALID. */
int mx_deck_waveform_view(int64_t pos_q32, uint32_t frames_per_px, uint32_t playhead_x, int64_t* first_frame);
/* Render the deck's current column analysis under *p into a new frame, asynchronous on `stream` (ORDER).  Refusals, in this order: a deck without a column analysis
 * MX_ERR_INVALID; settings the check refuses MX_ERR_INVALID; memory MX_ERR_NOMEM.  In each case *out is untouched and the deck stands as it was. */
struct mx_dframe;   /* the pixel path's device frame, below */
int mx_deck_render_waveform(mx_deck* d, const mx_deck_waveform* p, struct mx_dframe** out, void* stream);
/* Host only, pure: the same picture in plain C++ from n_cols records of an analysis at `column` of a track of n_frames (n_cols = ceil(n_frames / column), otherwise
 * MX_ERR_INVALID): the visible area alone -- w bytes of each of h rows at y, w / 2 bytes of each of h / 2 rows at u and v; bytes beyond it are not touched.  Strides
 * below the visible width, settings the check refuses, a column or n_frames ANALYSIS refuses, NULL: MX_ERR_INVALID.  How the rules are tested without a device. */
int mx_deck_waveform_host(const mx_deck_column* cols, uint64_t n_cols, uint32_t column, uint64_t n_frames, const mx_deck_waveform* p,
                          uint8_t* y, int32_t y_stride, uint8_t* u, uint8_t* v, int32_t c_stride);
/* DEBUG: what the last mx_deck_render_waveform of this process launched, in strips of MX_WAVE_STRIP pixel columns (a workgroup each): out[0] strips whose pixel columns
 * each held at most one record (and at least one of them one), out[1] strips that reduced several records in some pixel column, out[2] strips wholly outside the track,
 * out[3] the largest number of records one strip read.  Tests use it to know every form ran. */
int mx_deck_debug_last_waveform(uint32_t out[4]);

/* ---------------------------------------------------------------------------------------------- */
/* pixel path: device-resident yuv420p frames, VideoMixer, scaler, colour                          */
/* ---------------------------------------------------------------------------------------------- */

/* Host view of a frame: planar yuv420p, 8 bit (always, src/module/video_mixer.rs:282-283). */
typedef struct {
    uint32_t width, height;          /* luma size */
    uint8_t* data[3];                /* AVFrame.data   (codec/src/ffmpeg/frame.rs:188-197) */
    int32_t stride[3];               /* AVFrame.linesize */
    int64_t dur_num, dur_den;        /* video::Frame.duration_hint (src/video.rs:8-14) */
    int64_t off_num, off_den;        /* VideoFrame.tick_offset (src/engine/io.rs:12-17) */
} mx_frame;

/* Pixel formats a device frame can hold (codec/src/ffmpeg/pixfmt.rs:8-36 wraps AVPixelFormat; planar 8-bit YUV here).  Everything the
 * VideoMixer PRODUCES is yuv420p (src/module/video_mixer.rs:282-283); its INPUTS carry their own format in their picture settings and
 * the DynamicScaler's context converts implicitly (codec/src/ffmpeg/scale.rs:16-39, src/video/encode.rs:342-352: the settings compare
 * unequal when only the format differs).  Here that conversion is the build-specified scaler applied per plane: each chroma plane is
 * resampled from ITS size to the output's chroma size (DESIGN.md "Scaler" -- parity unpinned, like the scaler itself). */
typedef enum { MX_PIXFMT_YUV420P = 0, MX_PIXFMT_YUV422P = 1, MX_PIXFMT_YUV444P = 2,
               MX_PIXFMT_NV12 = 3 /* semi-planar 4:2:0, what hardware decoders deliver: plane 1 = interleaved U,V rows of `width` bytes, no plane 2
                                     (mx_frame.data[2] is ignored, mx_dframe_planes reports it NULL) */,
               /* packed RGB, one plane (data[0]; data[1], data[2] NULL): scaler INPUTS only (a screen capture, an image file).  BUILD-SPECIFIED: the
                * frame stands for the yuv444p frame of its per-pixel BT.709 limited-range conversion (DESIGN.md "Pixel formats"), which is then
                * resampled like any 4:4:4 input -- libswscale's own RGB path is unknown here: parity unpinned, like the scaler */
               MX_PIXFMT_RGB24 = 4 /* R, G, B bytes */, MX_PIXFMT_BGRA = 5 /* B, G, R, A bytes; A = the pixel's coverage, see MX_PIXFMT_YUVA420P */,
               /* the other planar 8-bit YUV layouts an AVPixelFormat descriptor can carry (pixfmt.rs:97-111: log2_chroma_w / log2_chroma_h of 0, 1 or 2): scaler
                * inputs like yuv422p / yuv444p -- every plane resampled from its own size; width / height multiples of the subsampling */
               MX_PIXFMT_YUV410P = 6 /* chroma 1/4 x 1/4 */, MX_PIXFMT_YUV411P = 7 /* chroma 1/4 x 1 */, MX_PIXFMT_YUV440P = 8 /* chroma 1 x 1/2 */,
               MX_PIXFMT_GRAY8 = 9 /* one plane of luma: stands for the yuv444p frame with U = V = 0x80 (scaler input only, like packed RGB) */,
               /* YUV deeper than 8 bits, as decoders of 10- / 12-bit streams deliver it (pixfmt.rs:107-111: bits per component from the descriptor): samples are 16-bit
                * little-endian words, mx_frame strides in BYTES as ever.  Scaler INPUTS only.  BUILD-SPECIFIED: the frame stands for the 8-bit frame of the same layout
                * whose samples are min(255, (v + 2^(b-9)) >> (b - 8)), v the b-bit value -- rounded to nearest, ties up: (v + 2) >> 2 for ten bits -- which is then
                * resampled like any 8-bit input (libswscale keeps the extra bits through its filters and dithers on the way out: unknown here, parity unpinned like the scaler) */
               MX_PIXFMT_YUV420P10 = 10, MX_PIXFMT_YUV422P10 = 11, MX_PIXFMT_YUV444P10 = 12 /* three planes, the value in the LOW ten bits of a word (the upper six ignored) */,
               MX_PIXFMT_P010 = 13 /* semi-planar 4:2:0 like nv12: luma plane + one plane of interleaved U,V words, the value in the HIGH ten bits of a word (the lower six ignored) */,
               MX_PIXFMT_YUV420P12 = 14, MX_PIXFMT_YUV422P12 = 15, MX_PIXFMT_YUV444P12 = 16 /* the value in the low twelve bits (the upper four ignored) */,
               MX_PIXFMT_YUV420P16 = 17, MX_PIXFMT_YUV422P16 = 18, MX_PIXFMT_YUV444P16 = 19 /* all sixteen bits */,
               MX_PIXFMT_P016 = 20 /* semi-planar 4:2:0, all sixteen bits (p012 is this layout with the low four bits zero: the same rounding applies) */,
               /* packed 4:2:2, one plane of 2 bytes per pixel (what capture devices deliver): scaler INPUTS only; the frame stands for the yuv422p frame with the same
                * samples (a byte shuffle, nothing to specify), which is then resampled like any yuv422p input; width even */
               MX_PIXFMT_YUYV422 = 21 /* Y0 U Y1 V */, MX_PIXFMT_UYVY422 = 22 /* U Y0 V Y1 */,
               /* the other byte orders of packed 8-bit RGB: the same build-specified conversion as rgb24 / bgra */
               MX_PIXFMT_BGR24 = 23 /* B, G, R */, MX_PIXFMT_RGBA = 24 /* R, G, B, A */, MX_PIXFMT_ARGB = 25 /* A, R, G, B */, MX_PIXFMT_ABGR = 26 /* A, B, G, R */,
               /* PER-PIXEL ALPHA (BUILD-SPECIFIED: the reference's only "alpha" is the VideoMixer's global fader, video_mixer.rs:168).  A layer may carry a COVERAGE
                * plane -- yuva420p: yuv420p plus a fourth plane of width x height bytes, 255 = opaque (mx_frame holds the three YUV planes; the fourth travels through
                * mx_dframe_upload_alpha / _download_alpha) -- and the A byte of a four-byte packed RGB input IS that plane (straight, not premultiplied).  The scaler
                * resamples it like luma (letterbox bars opaque).  A VideoMixer step then weighs its layers per sample, in fade_line's own u16 arithmetic
                * (video_mixer.rs:211-235), aA / aB = the coverage of A / B there (255 where a layer carries none; chroma samples use the co-sited luma sample's):
                *     wa = (aA * fade) / 255;   wb = (aB * (255 - wa)) / 255;   out = (A * (255 - wb) + B * wb) / 255
                * Opaque layers give wa = fade, wb = 255 - fade: the reference's cross-fade bit for bit.  The composite itself is opaque yuv420p (DESIGN.md "Per-pixel alpha"). */
               MX_PIXFMT_YUVA420P = 27 } mx_pixfmt;

/* Device frame: the AvFrame<Video> stand-in.  Reference-counted like an AVFrame (clone =
 * av_frame_clone, codec/src/ffmpeg/frame.rs:351-361): create returns one reference; the VideoMixer
 * keeps inputs past the call by retaining them.  Frames are immutable once handed to a mixer.
 * All stateless pixel calls take a hipStream_t (`stream`, NULL = the library's default video
 * stream) and are asynchronous on it unless stated. */
typedef struct mx_dframe mx_dframe;
int mx_dframe_create(uint32_t width, uint32_t height, void* stream, mx_dframe** out);  /* yuv420p; blank: Y=0 U=V=0x80 (frame.rs:76-138) */
/* any mx_pixfmt: width / height must be multiples of the chroma subsampling (pixfmt.rs:97-111); mx_frame planes follow the device frame's format */
int mx_dframe_create_fmt(uint32_t width, uint32_t height, mx_pixfmt fmt, void* stream, mx_dframe** out);
int mx_dframe_format(const mx_dframe* f, mx_pixfmt* fmt);
int mx_dframe_retain(mx_dframe* f);
void mx_dframe_release(mx_dframe* f);
int mx_dframe_upload(mx_dframe* f, const mx_frame* host, void* stream);       /* visible area; synchronous */
int mx_dframe_download(const mx_dframe* f, mx_frame* host, void* stream);     /* visible area; synchronous */
int mx_dframe_planes(const mx_dframe* f, uint32_t* width, uint32_t* height, void* device_data[3], int32_t stride[3]);
/* The coverage plane of a yuva420p frame (MX_PIXFMT_YUVA420P): width x height bytes, `stride` bytes per host row.  Synchronous.  MX_ERR_INVALID for a frame
 * without one.  alpha_plane: its device address (NULL: none) for producers that write it on the device. */
int mx_dframe_upload_alpha(mx_dframe* f, const uint8_t* host_alpha, int32_t stride, void* stream);
int mx_dframe_download_alpha(const mx_dframe* f, uint8_t* host_alpha, int32_t stride, void* stream);
int mx_dframe_alpha_plane(const mx_dframe* f, void** device_alpha, int32_t* stride);

/* AvFrame::blank (frame.rs:76-138) */
int mx_video_blank(mx_dframe* f, void* stream);
/* The compose step of VideoMixer::run_tick (src/module/video_mixer.rs:150-239): out = cross-fade of
 * a and b by `(fader * 255.0) as u8`; a/b NULL reads the blank plane (video_mixer.rs:180-188). */
int mx_video_crossfade(mx_dframe* out, const mx_dframe* a, const mx_dframe* b, double fader, void* stream);
/* DynamicScaler::scale (src/video/encode.rs:338-397) of `in` into `out`'s size: identity copy when
 * equal, else blank + aspect-preserving letterboxed bicubic.  The bicubic arithmetic is
 * BUILD-SPECIFIED (libswscale is outside the reference tree): see DESIGN.md "Scaler". */
int mx_video_scale(const mx_dframe* in, mx_dframe* out, void* stream);
/* DynamicScaler (src/video/encode.rs:338-397): keeps its context (tap tables, blank letterboxed output frame) while the
 * input settings stay the same -- what Monitor / StreamOutput call once per tick to shrink the program frame before it
 * leaves the device (monitor.rs:21-22, stream_output.rs:23-24, encode.rs:287-295).  *out holds one reference
 * (mx_dframe_release); it is the input itself when the sizes are equal (encode.rs:342-345), else the scaler's own frame,
 * overwritten by the next call.  Asynchronous on the scaler's stream. */
typedef struct mx_video_scaler mx_video_scaler;
int mx_video_scaler_create(uint32_t out_width, uint32_t out_height, void* stream, mx_video_scaler** out);
int mx_video_scaler_scale(mx_video_scaler* sc, const mx_dframe* in, mx_dframe** out);
void mx_video_scaler_destroy(mx_video_scaler* sc);
int mx_video_scale_geometry(uint32_t in_w, uint32_t in_h, uint32_t out_w, uint32_t out_h,
                            uint32_t* scaled_w, uint32_t* scaled_h, uint32_t* letterbox_x, uint32_t* letterbox_y);   /* encode.rs:354-374 */
/* Row band of DynamicScaler::scale for a picture composited over several GPUs by rows (mixlab_amd/shard.py):
 * luma rows [row0, row0 + out_band height) of the (full_w x full_h) letterboxed result, computed from a SLICE that holds luma rows
 * [src_row0, src_row0 + slice height) of a source in_full_h rows high.  Tap indices clamp against the full source plane, exactly as
 * the unsharded scale does, so stitched bands are the unsharded frame bit for bit; a slice that lacks a row the band's vertical
 * taps reach is MX_ERR_INVALID.  All row counts even (whole chroma rows); out_band is as wide as the full picture.  Synchronous. */
int mx_video_scale_band(const mx_dframe* in_slice, uint32_t in_full_h, uint32_t src_row0, mx_dframe* out_band,
                        uint32_t full_w, uint32_t full_h, uint32_t row0, void* stream);
/* The scaler's tap table for one axis (DESIGN.md "Scaler"): *n_taps coefficients (Q14, summing to 16384) per output sample and the
 * index of the first source sample each set applies to.  first: [dst], coef: [dst][*n_taps] with room for mx_video_scaler_tap_count()
 * entries per sample.  Host-only (no device needed): what the tests pin against tests/golden/bicubic_taps_*.json. */
uint32_t mx_video_scaler_tap_count(uint32_t src, uint32_t dst);
int mx_video_scaler_taps(uint32_t src, uint32_t dst, int32_t* first, int32_t* coef, uint32_t* n_taps);
/* BUILD-SPECIFIED (no reference counterpart): BT.709 limited-range YUV420P -> RGBA8 (+ optional Q12 3x4 matrix). */
int mx_video_to_rgba(const mx_dframe* in, void* device_rgba, int32_t rgba_stride, const int32_t* matrix_q12 /* 12 or NULL */, void* stream);
/* The KEYER (BUILD-SPECIFIED; the reference has none): a chroma or luma key computed on the device.  `in` is yuv420p or yuva420p
 * (anything else: MX_ERR_INVALID -- conversion is the scaler's business); *out is a NEW yuva420p frame of the same size carrying one reference.  Y is copied, U and V are
 * copied or spill-suppressed, the coverage plane is the key.  Stride padding is never read as picture.  Integer arithmetic throughout, `/` truncates:
 *   ramp(d; lo, hi) = 0 if d <= lo, else 255 if d >= hi, else ((d - lo) * 255) / (hi - lo)            (tests in this order: lo == hi is a hard key)
 *   CHROMA, per chroma sample:  du = U - key_u, dv = V - key_v;  d = floor(sqrt((du du + dv dv) << 8))  (the exact integer root: a distance in 1/16 code values, <= 5769)
 *     ac = ramp(d; near_q4, far_q4);  coverage of luma sample (x, y) = the 2x bilinear upsample, chroma co-sited with luma (2cx, 2cy):
 *     cx = x >> 1, cy = y >> 1, cx1 = min(cx + (x & 1), W/2 - 1), cy1 = min(cy + (y & 1), H/2 - 1);  k = (ac[cy][cx] + ac[cy][cx1] + ac[cy1][cx] + ac[cy1][cx1] + 2) >> 2
 *     (on even (x, y) k = ac[cy][cx]: the compositor's chroma samples, which take the coverage of luma (2x, 2y), read the keyer's own chroma decision back)
 *   LUMA, per luma sample:  k = ramp(Y * 16; near_q4, far_q4); chroma is copied
 *   both:  if invert, k = 255 - k;  if `in` carries coverage a_in, k = (k * a_in) / 255;  k is the output coverage byte
 *   SPILL (chroma mode, active iff spill_strength > 0 and spill_far_q4 > far_q4), per chroma sample, whatever `invert` is:
 *     w = ((255 - ramp(d; far_q4, spill_far_q4)) * spill_strength) / 255;  U' = 128 + tdiv((U - 128) * (255 - w), 255), V likewise (tdiv: signed, toward zero)
 * Values outside the ranges in the comments below are MX_ERR_INVALID.  Asynchronous on `stream`, like its neighbours. */
enum { MX_KEY_CHROMA = 0, MX_KEY_LUMA = 1 };
typedef struct {
    uint32_t mode;            /* MX_KEY_CHROMA or MX_KEY_LUMA */
    uint8_t  key_u, key_v;    /* chroma mode: the key colour */
    uint8_t  invert;          /* 0 or 1 */
    uint8_t  _pad;            /* 0 */
    uint32_t near_q4, far_q4; /* distances in 1/16 of a code value; near <= far <= 65535 */
    uint32_t spill_far_q4;    /* chroma mode; <= 65535 */
    uint32_t spill_strength;  /* 0 .. 255; must be 0 in luma mode */
} mx_video_key_params;        /* 24 bytes */
int mx_video_key(const mx_dframe* in, const mx_video_key_params* params, mx_dframe** out, void* stream);
/* The COLOUR CORRECTOR (BUILD-SPECIFIED; the reference has none): a luma curve, a chroma matrix and a 3D LUT applied to ONE frame in ONE launch
 * on the device -- what matches camera 2 to camera 1 once the scopes have shown the difference.  `in` is yuv420p or yuva420p (anything else: MX_ERR_INVALID); *out is a NEW
 * frame of the same size and the same format carrying one reference.  A coverage plane is copied byte for byte.  Stride padding is left as mx_dframe_create_fmt leaves it
 * and is never read as picture.  All quantities are integers; `>>` on a negative value is the arithmetic shift (floor); clip8 clamps to 0 .. 255.
 * The three stages run in this order, each switched by a flag bit; with no bit set the visible area is a copy.
 *   CURVE (MX_GRADE_CURVE), per luma sample:  y1 = curve_y[Y]  (a table of 256 bytes); without the bit y1 = Y.
 *   CHROMA (MX_GRADE_CHROMA), per chroma sample, du = U - 128, dv = V - 128:
 *     u1 = clip8(128 + ((m_uu du + m_uv dv + off_u + 2048) >> 12));  v1 = clip8(128 + ((m_vu du + m_vv dv + off_v + 2048) >> 12))
 *     coefficients Q12 with |m| <= 32767, offsets Q12 with |off| <= 255 * 4096: every sum fits an int32.  Without the bit u1 = U, v1 = V.
 *   LUT (MX_GRADE_LUT) needs an mx_video_lut: a lattice of N = 2^k + 1 nodes per axis, k = lattice_log2 in {4, 5} (N = 17 or 33).  The node at (iy, iu, iv) is three
 *     uint16 (Y', U', V') in Q4, each 0 .. 4096 (4096 stands for code value 256, so the top node of the identity is exact; a larger value is MX_ERR_INVALID at
 *     creation), stored at nodes[((iy N + iu) N + iv) 3 + c].  With sh = 8 - k and S = 2^sh, the evaluation at (a, b, c) = (Y, U, V):
 *       the cell is (a >> sh, b >> sh, c >> sh), the fractions f = (a & (S-1), b & (S-1), c & (S-1));  TETRAHEDRAL interpolation: order the axes by fraction,
 *       f1 >= f2 >= f3; walk from the cell's low corner one step along the axis of f1, then of f2, then of f3: nodes n0 .. n3, weights S - f1, f1 - f2, f2 - f3, f3
 *       (equal fractions give the vertex they would disagree on the weight 0: no tie rule is needed);  per output channel acc = sum w_i n_i[ch] (<= 65536) and the
 *       result is min(255, (acc + 8 S) >> (sh + 4)).  The identity lattice (node = 16 S index per axis) returns its input exactly.
 *     LUMA sample (x, y):  Y' = LUT_Y(y1, u1[y>>1][x>>1], v1[y>>1][x>>1]) -- the chroma of its own 2 x 2 block, no upsample.
 *     CHROMA sample (cx, cy):  (U', V') = LUT_UV(ym, u1, v1) with ym = (y1[2cy][2cx] + y1[2cy][2cx+1] + y1[2cy+1][2cx] + y1[2cy+1][2cx+1] + 2) >> 2, the block's mean
 *     of the CURVED luma.  Without the bit Y' = y1, U' = u1, V' = v1.
 * A flag bit outside the three, a coefficient or offset out of range, the LUT bit without a LUT and a LUT without the bit are MX_ERR_INVALID.  Asynchronous on `stream`,
 * like its neighbours.  Out of scope: the grade on a band-scaled source and on mixer output ports, other pixel formats, 65-point lattices, and reading .cube files (the
 * host resamples them to the lattice). */
enum { MX_GRADE_CURVE = 1, MX_GRADE_CHROMA = 2, MX_GRADE_LUT = 4 };
typedef struct {
    uint32_t flags;                                  /* MX_GRADE_* bits */
    uint8_t  curve_y[256];
    int32_t  m_uu, m_uv, m_vu, m_vv, off_u, off_v;   /* Q12 */
} mx_video_grade_params;                             /* 284 bytes */
typedef struct mx_video_lut mx_video_lut;            /* immutable, reference-counted, uploaded once at creation */
int  mx_video_lut_create(uint32_t lattice_log2, const uint16_t* nodes /* [N][N][N][3] */, mx_video_lut** out);   /* one reference for the caller; checks come before any device work */
int  mx_video_lut_retain(mx_video_lut* lut);
void mx_video_lut_release(mx_video_lut* lut);
int  mx_video_lut_identity(uint32_t lattice_log2, uint16_t* nodes /* [N][N][N][3] */);   /* host only */
/* Host only, f64: curve_y[i] = clip8(rint(255 * clamp((i - black) / (white - black), 0, 1) ^ (1 / gamma))), the matrix rint(4096 * saturation * [[cos h, sin h],
 * [-sin h, cos h]]) (rows u, v), zero offsets, flags CURVE | CHROMA.  MX_ERR_INVALID for white <= black, gamma <= 0 or a coefficient outside +-32767;
 * (0, 255, 1, 1, 0) gives the identity table and 4096 * I exactly. */
int  mx_video_grade_procamp(double black, double white, double gamma, double saturation, double hue_degrees, mx_video_grade_params* out);
int  mx_video_grade(const mx_dframe* in, const mx_video_grade_params* params, const mx_video_lut* lut /* NULL iff the LUT bit is clear */, mx_dframe** out, void* stream);
/* The MATTE REFINER (BUILD-SPECIFIED; the reference has none): the knobs behind a keyer -- clean (clip), choke (shrink / grow), soften -- and
 * a garbage mask, applied to the coverage plane of ONE frame in ONE launch on the device.  A rectangle or a circle written into layer B's coverage with the
 * VideoMixer's fader at rest on 0 is a wipe or an iris: out = (A (255 - aB) + B aB) / 255 through the compositor as it stands.
 * `in` is yuv420p or yuva420p, W x H (anything else: MX_ERR_INVALID); *out is a NEW yuva420p frame of the same size carrying one reference.  Y, U and V are copied
 * byte for byte; the coverage plane is computed as below from A_in, the input's coverage, or 255 everywhere without one.  Stride padding is never read as picture,
 * and the output's padding is what mx_dframe_create_fmt leaves.  Everything is an integer; `/` truncates, `>>` is of a non-negative value.
 * Every field of a stage whose flag bit is clear must be 0 and anything out of the ranges stated with the fields is MX_ERR_INVALID; with no bit set the frame is
 * copied, with an opaque plane where the input had none.  The stages run in this order, each per luma sample (x, y); a stage that is off passes its input on:
 *   CLEAN:  a1 = 0 if A_in <= clean_black; else 255 if A_in >= clean_white; else ((A_in - clean_black) 255) / (clean_white - clean_black).  The tests are made in
 *     this order, so black == white is a hard clip and (0, 255) is the identity.
 *   CHOKE, r = |choke|:  a2(x, y) = the minimum (choke > 0, the matte shrinks) or the maximum (choke < 0, it grows) of a1(cl(x + i, W), cl(y + j, H)) over
 *     |i|, |j| <= r, with cl(t, n) = min(max(t, 0), n - 1): a square window clamped to the plane.
 *   SOFTEN, s = soften, b_s[k] = C(2s, k + s) for k = -s .. s (sum 4^s):
 *     a3(x, y) = (sum_j sum_i b_s[j] b_s[i] a2(cl(x + i, W), cl(y + j, H)) + 2^(4s - 1)) >> 4s -- ONE rounding, at the end.  The largest sum is 255 2^24 < 2^32:
 *     that is why 6 is the limit and why the two passes of a separable form need no rounding between them.
 *   MASK, with px = 16 x + 8, py = 16 y + 8 (the sample's centre in Q4 luma pixels):
 *     RECT:    d = min(px - x0, x1 - px, py - y0, y1 - py)
 *     CIRCLE:  d = x1 - isqrt((px - x0)^2 + (py - y0)^2), isqrt the EXACT floor of the root (the argument stays below 2^43)
 *     m = 0 if d <= 0; else 255 if d >= mask_feather_q4; else (d 255) / mask_feather_q4 -- in this order, so feather 0 is a hard edge; the feather lies inside
 *     the shape.  If mask_invert, m = 255 - m.  The result is (a3 m) / 255.
 * Coverage is decided per luma sample; the compositor's rule that a chroma sample takes the coverage of luma (2x, 2y) stands.  Asynchronous on `stream`, like its
 * neighbours.  Out of scope: the refiner on mixer output ports and on band-scaled sources, other shapes (ellipse, diamond, line) and other structuring elements,
 * radii above 6, temporal smoothing, and a wipe setting inside the VideoMixer. */
#define MX_MATTE_CLEAN 1u
#define MX_MATTE_CHOKE 2u
#define MX_MATTE_SOFTEN 4u
#define MX_MATTE_MASK 8u
#define MX_MATTE_MASK_RECT 0u
#define MX_MATTE_MASK_CIRCLE 1u
typedef struct {
    uint32_t flags;                      /* MX_MATTE_* bits, no other */
    uint8_t  clean_black, clean_white;   /* CLEAN: black <= white */
    int8_t   choke;                      /* CHOKE: -6 .. 6, not 0; > 0 shrinks, < 0 grows */
    uint8_t  soften;                     /* SOFTEN: 1 .. 6 */
    uint32_t mask_shape, mask_invert;    /* MASK: RECT | CIRCLE; 0 | 1 */
    int32_t  mask_x0, mask_y0, mask_x1, mask_y1;   /* Q4 luma pixels, |.| <= 2^20.  RECT: the edges, x0 <= x1, y0 <= y1.  CIRCLE: centre (x0, y0), radius x1 >= 0, y1 = 0 */
    uint32_t mask_feather_q4;            /* 0 .. 65535 */
} mx_video_matte_params;                 /* 36 bytes */
int mx_video_matte(const mx_dframe* in, const mx_video_matte_params* params, mx_dframe** out, void* stream);
/* Host only: the parameter checks of mx_video_matte alone (MX_OK or MX_ERR_INVALID, mx_last_error saying which rule), made before any device work. */
int mx_video_matte_check(const mx_video_matte_params* params);
/* Host only: a MASK-only setting for a wipe of a w x h frame at position pos (0 .. 65536) with feather f = feather_q4 (0 .. 65535), in 64-bit integers, B = 2^20:
 *   LEFT:  RECT (-B, -B, (pos (16 w + f)) >> 16, B);   TOP:  RECT (-B, -B, B, (pos (16 h + f)) >> 16);
 *   BOX:   hx = (pos (8 w + f)) >> 16, hy = (pos (8 h + f)) >> 16, RECT (8 w - hx, 8 h - hy, 8 w + hx, 8 h + hy);
 *   IRIS:  CIRCLE at (8 w, 8 h), radius (pos (isqrt((8 w)^2 + (8 h)^2) + 1 + f)) >> 16.
 * pos = 0 covers nothing and pos = 65536 leaves every sample at 255.  MX_ERR_INVALID for another kind, pos or feather out of range, or a size that is not even,
 * non-zero and at most 16384. */
#define MX_WIPE_LEFT 0u
#define MX_WIPE_TOP 1u
#define MX_WIPE_BOX 2u
#define MX_WIPE_IRIS 3u
int mx_video_matte_wipe(uint32_t kind, uint32_t pos, uint32_t feather_q4, uint32_t w, uint32_t h, mx_video_matte_params* out);
/* The PLACER (BUILD-SPECIFIED; the reference has none): a crop of a frame resampled into a rectangle of a transparent canvas, on the device --
 * picture-in-picture, side-by-side, a keyed presenter in a corner, a zoom.  `in` is yuv420p or yuva420p (anything else: MX_ERR_INVALID -- conversion is the scaler's
 * business); *out is a NEW yuva420p frame of canvas_w x canvas_h carrying one reference, its stride padding as mx_dframe_create_fmt leaves it.  The input's padding, and
 * input samples outside the crop, are never read as picture.  All quantities are integers.
 *   CROP PLANES: Y and the input coverage A_in restricted to [crop_x, crop_x + crop_w) x [crop_y, crop_y + crop_h); U and V restricted to the same rectangle with every
 *     number halved.
 *   RESAMPLED PLANES Sy, Su, Sv, Sa: the crop planes resampled exactly as the scaler (DESIGN.md "Scaler", mx_video_scaler_taps) resamples a frame that consisted of the
 *     crop alone: tap tables (crop_w -> dst_w, crop_h -> dst_h) for luma and coverage, (crop_w/2 -> dst_w/2, crop_h/2 -> dst_h/2) for chroma; H pass over every crop
 *     row t = (sum hc * S + 64) >> 7; V pass clip8((sum vc * t + 2^20) >> 21); tap indices clamp to the CROP, not to the plane.  No letterbox and no aspect rule: the crop
 *     is stretched to the rectangle (mx_video_scale_geometry is the caller's tool to keep an aspect).  Without input coverage Sa is 255 everywhere.
 *   CANVAS: luma and coverage at (x, y) are Sy, Sa at (x - dst_x, y - dst_y) when dst_x <= x < dst_x + dst_w and dst_y <= y < dst_y + dst_h, otherwise Y = 0 and
 *     coverage = 0.  Chroma at (cx, cy) is Su, Sv at (cx - dst_x/2, cy - dst_y/2) inside the halved rectangle, otherwise 0x80.  The tables are always those of the full
 *     dst_w x dst_h, however much of the rectangle the canvas clips away; a rectangle wholly outside the canvas gives a blank, fully transparent frame and is no error.
 *     Every number being even, a chroma sample's co-sited luma sample (2cx, 2cy) is inside the rectangle exactly when the chroma sample is: the compositor's coverage
 *     rule for chroma needs nothing new.
 * Values outside the ranges in the comments below are MX_ERR_INVALID; so is a crop that does not lie inside `in`.  Stateless; asynchronous on `stream`, like mx_video_key. */
typedef struct {
    uint32_t canvas_w, canvas_h;               /* even, >= 2, within what mx_dframe_create_fmt accepts */
    uint32_t crop_x, crop_y, crop_w, crop_h;   /* even; crop_w = crop_h = 0 (then crop_x = crop_y = 0): the whole frame; otherwise >= 2 and inside the input frame */
    int32_t  dst_x, dst_y;                     /* even; may be negative or beyond the canvas: the rectangle is clipped */
    uint32_t dst_w, dst_h;                     /* even, >= 2, <= 16384; crop_w <= 32 * dst_w and crop_h <= 32 * dst_h (at most 130 taps per axis, mx_video_scaler_tap_count) */
} mx_video_place_params;                       /* 40 bytes */
int mx_video_place(const mx_dframe* in, const mx_video_place_params* params, mx_dframe** out, void* stream);
/* The MULTIVIEWER (BUILD-SPECIFIED; the reference shows several pictures with one MSE Monitor per module): up to MX_MULTIVIEW_MAX frames, each
 * resampled into its own rectangle ("view") of ONE opaque canvas with a tally frame round it, in ONE launch that writes every byte of the canvas once -- the A / B / program
 * and input thumbnails of a vision mixer side by side, red round what is on air, green round the preview.  All quantities are integers.
 *   VIEW i has the rectangle R = (x, y, w, h) on the canvas, frame included.  Views must not overlap, frames included (touching is allowed).
 *   INNER RECTANGLE I: R inset by `border` on all four sides.  PICTURE RECTANGLE P: with fit = 0, P = I; with fit = 1,
 *     (sw, sh, lx, ly) = mx_video_scale_geometry(src_w, src_h, I.w, I.h) (the DynamicScaler's rule, encode.rs:354-374) and P is sw x sh at (I.x + lx, I.y + ly).
 *   SHOWN: view i is shown when its frame is present (in[i] != NULL), the frame is yuv420p or yuva420p, P.w >= 2 and P.h >= 2, and src_w <= 32 P.w and
 *     src_h <= 32 P.h (the placer's limit of 130 taps per axis).  A view that is not shown is no error -- it depends on the frames that arrive; bit i of the
 *     shown mask says which views were shown.
 *   CANVAS LUMA at (x, y): outside every view's rectangle bg_y; inside a view's R but outside its I border_y; inside I but outside P -- or anywhere in I of a view
 *     that is not shown -- 0, the scaler's blank (frame.rs:76-138); inside P of a shown view Sy at (x - P.x, y - P.y), where Sy is the WHOLE source luma plane
 *     resampled to P.w x P.h exactly as mx_video_place's RESAMPLED PLANES with a whole-frame crop: tables (src_w -> P.w, src_h -> P.h) of DESIGN.md "Scaler"
 *     (mx_video_scaler_taps), H pass t = (sum hc * S + 64) >> 7 over every source row, V pass clip8((sum vc * t + 2^20) >> 21), tap indices clamped to the
 *     plane's visible area.
 *   CANVAS CHROMA: the same with every number halved -- tables (src_w/2 -> P.w/2, src_h/2 -> P.h/2), blank 0x80, border_u / border_v, bg_u / bg_v.
 *   COVERAGE: a source's coverage plane is IGNORED: a multiviewer shows the source, not its key.  Honouring it (a view over a background picture) is a stated follow-up.
 *   OUTPUT: *out is a NEW opaque yuv420p frame of canvas_w x canvas_h carrying one reference, its stride padding as mx_dframe_create leaves it (Y 0, chroma 0x80).
 *     The inputs' padding is never read as picture.
 * Consequences: with fit = 1, I of a shown view is byte for byte what mx_video_scale writes into an I.w x I.h frame; with fit = 0, P equals the Y / U / V of
 * mx_video_place of the whole frame into that rectangle.
 * Overlapping views, or any value outside the ranges in the comments below, are MX_ERR_INVALID -- checked on the host before any device is touched.
 * Stateless; asynchronous on `stream`, like mx_video_place. */
#define MX_MULTIVIEW_MAX 16
typedef struct {
    uint32_t x, y, w, h;                     /* the view's rectangle on the canvas, frame included: even, inside the canvas, w and h >= 2 * border + 2 */
    uint32_t border;                         /* even, 0 .. 64: thickness of the tally frame */
    uint8_t  border_y, border_u, border_v;   /* its colour */
    uint8_t  fit;                            /* 0: stretch to the inner rectangle; 1: keep the aspect (mx_video_scale_geometry) */
} mx_multiview_view;                         /* 24 bytes */
typedef struct {
    uint32_t canvas_w, canvas_h;             /* even, >= 2, within what mx_dframe_create_fmt accepts */
    uint8_t  bg_y, bg_u, bg_v, _pad;         /* the canvas outside every view; _pad 0 */
    uint32_t n_views;                        /* 1 .. MX_MULTIVIEW_MAX */
    uint32_t hop;                            /* graph form only, >= 1; the pixel call ignores it */
    mx_multiview_view view[MX_MULTIVIEW_MAX];/* entries beyond n_views are not looked at */
} mx_multiview_params;                       /* 404 bytes */
int mx_video_multiview(const mx_dframe* const* in /* [n_views], NULL = no frame */, const mx_multiview_params* params,
                       mx_dframe** out, uint32_t* shown_mask /* may be NULL */, void* stream);
int mx_video_sync(void* stream);
/* A caller-owned hipStream_t that graphs / scalers / mixers launched pictures on is about to be destroyed: release what the library keeps per (device, stream) for its
 * batched video launches (page-locked descriptor staging, device copies, events, an upload stream).  The library frees this itself for streams it created; for a caller's
 * stream it cannot know when the stream dies -- and a later stream may be given the same handle value.  Call it after the last launch on the stream has finished
 * (it synchronises the upload stream, not `stream`). */
int mx_stream_retired(void* stream);

/* VideoMixer (src/module/video_mixer.rs): 4 video inputs, program + A + B outputs. */
typedef struct { mx_dframe* frame; /* NULL = no frame this tick */ int64_t dur_num, dur_den, off_num, off_den; } mx_video_input;
typedef struct mx_video_mixer mx_video_mixer;
int mx_video_mixer_create(const mx_video_mixer_params* params, uint32_t sample_rate /* 0 => 44100 */, void* stream, mx_video_mixer** out);
int mx_video_mixer_update(mx_video_mixer* m, const mx_video_mixer_params* params);
/* One VideoMixer::run_tick (video_mixer.rs:70-250).  Returned frames carry one reference for the
 * caller (mx_dframe_release when done); NULL = None.  The program frame has duration 1/60 and
 * tick_offset 0 (video_mixer.rs:241-247).  The pixels are produced asynchronously on the mixer's stream (mx_video_mixer_create; NULL = the
 * library's default video stream, the one every entry point with a NULL stream uses): consume them there, or mx_video_mixer_sync first. */
int mx_video_mixer_run_tick(mx_video_mixer* m, uint64_t t, const mx_video_input inputs[4],
                            mx_dframe** out_program, mx_dframe** out_a, mx_dframe** out_b);
int mx_video_mixer_sync(mx_video_mixer* m);
void mx_video_mixer_destroy(mx_video_mixer* m);

/* Video nodes inside a graph (MX_KIND_VIDEO_MIXER / SOURCE_VIDEO / VIDEO_TO_RGBA): every tick of
 * mx_graph_run_ticks runs the video sub-graph in run order, all launches on the graph's stream.
 * set_video_source: the frame the source emits -- on the next tick only (repeat = 0, like one
 * decoded frame arriving, media_source.rs:93-126) or as a new frame on every tick (repeat = 1,
 * synthetic 60 fps input).  frame NULL clears it.  The graph retains the frame. */
int mx_graph_set_video_source(mx_graph* g, uint32_t node, mx_dframe* frame, int64_t dur_num, int64_t dur_den,
                              int64_t off_num, int64_t off_den, int repeat);
/* A source that delivers a NEW frame on every tick, cycling through `n` frames (a decoder feeding the graph: MediaSource emits
 * at most one VideoFrame per tick, media_source.rs:93-126): the k-th tick on which the ring delivers, counted from 0 at this call, emits
 * frames[k mod n] with the given duration hint and offset.  The count is carried across runs and does not depend on first_tick; a tick on which
 * queued frames (mx_graph_queue_video_source) take the ring's place does not advance it -- a decoder that was not asked delivers its next frame
 * when it is asked again.  A call with n > 0 drops a set frame (mx_graph_set_video_source).  The graph retains the frames.  n = 0 clears the source. */
int mx_graph_set_video_source_ring(mx_graph* g, uint32_t node, mx_dframe* const* frames, size_t n, int64_t dur_num, int64_t dur_den,
                                   int64_t off_num, int64_t off_den);
/* Row-band sharding of one composited picture over ranks (mixlab_amd/shard.py): a rank's graph is the cascade at (full_w x
 * band_rows).  Layers of the picture's own size are fed as their band rows; a SMALLER layer is fed as the halo slice its band needs
 * (luma rows [src_row0, src_row0 + slice_rows) of an in_w x in_full_h yuv420p source, shard.band_source_rows) and this call makes
 * the source node deliver, on every tick it has a frame, luma rows [row0, row0 + band_rows) of that layer's letterboxed scale into
 * (full_w x full_h) -- what DynamicScaler::scale (encode.rs:338-397) gives the unsharded VideoMixer, cut to the band; asynchronous,
 * on the graph's stream.  band_rows = 0 removes the transform. */
int mx_graph_set_video_source_band(mx_graph* g, uint32_t node, uint32_t in_w, uint32_t in_full_h, uint32_t src_row0, uint32_t slice_rows,
                                   uint32_t full_w, uint32_t full_h, uint32_t row0, uint32_t band_rows);
/* The keyer as a per-source transform (mx_video_key): on every tick the SOURCE_VIDEO node has a frame -- from mx_graph_set_video_source, _ring,
 * mx_graph_queue_video_source, and therefore mx_media_source_feed / mx_stream_input_feed -- it delivers the keyed yuva420p frame instead, computed on the graph's stream
 * before the tick's video work.  Frames are immutable, so a frame is keyed once per setting and the result reused while anything still holds the frame (a repeated frame,
 * or a ring of n frames, costs n launches, not one per tick); a pooled output frame is rewritten only when nothing else holds a reference to it.  params NULL removes the
 * transform.  MX_ERR_TYPE for a node that is not a SOURCE_VIDEO, MX_ERR_INVALID for bad parameters and together with mx_graph_set_video_source_band (a band-scaled layer
 * cannot carry coverage).  A source frame that is not yuv420p / yuva420p fails the run with MX_ERR_INVALID, mx_last_error naming the node.  A scope tap on the source's
 * port sees the keyed frame.  mx_graph_adopt_state does not carry the setting. */
int mx_graph_set_video_source_key(mx_graph* g, uint32_t node, const mx_video_key_params* params /* NULL removes */);
/* The placer as a per-source transform (mx_video_place): on every tick the SOURCE_VIDEO node has a frame -- from any of the feeders listed above --
 * it delivers the placed yuva420p canvas instead.  With a key set on the same node the order is KEY, THEN PLACE, whichever call came first: the key is decided at the source's
 * own resolution and its coverage is resampled with the picture.  The keyer's cache and pool rules hold: a frame is transformed once per setting, not once per tick, and a
 * pooled output is rewritten only when the pool alone holds it; the tap tables are uploaded once per setting (and per size of a whole-frame crop), not per frame.  params NULL
 * removes the transform.  MX_ERR_TYPE for a node that is not a SOURCE_VIDEO, MX_ERR_INVALID for bad parameters and together with mx_graph_set_video_source_band, in either
 * order.  A source frame of another format, or a crop outside the frame that arrives, fails the run with MX_ERR_INVALID, mx_last_error naming the node, before anything of the
 * run is launched.  A scope tap on the source's port sees the placed frame.  mx_graph_adopt_state does not carry the setting. */
int mx_graph_set_video_source_place(mx_graph* g, uint32_t node, const mx_video_place_params* params /* NULL removes */);
/* The matte refiner as a per-source transform (mx_video_matte), under the keyer's rules: it applies to every frame the SOURCE_VIDEO node
 * delivers, whichever feeder brought it; a frame is refined once per setting and the result reused (a ring of n frames costs n launches, not one per tick; the 32 most
 * recent pairs are kept); output frames come from a pool and are rewritten only when the pool alone holds them.  Where several transforms are set on a node the order is
 * GRADE, THEN KEY, THEN MATTE, THEN PLACE, whatever the call order: the matte refines what the key decided and the placer resamples the refined plane.  A scope tap on
 * the source's port sees the matted frame.  Setting it again (a wipe moving every tick) drops what every stage had cached, from the next run on; params NULL removes
 * the transform.  MX_ERR_TYPE for a node that is not a SOURCE_VIDEO; MX_ERR_INVALID for whatever mx_video_matte_check refuses, and together with
 * mx_graph_set_video_source_band, in either call order (mx_last_error names the other setting); each leaves the graph usable.  A source frame that is not yuv420p /
 * yuva420p fails the run with MX_ERR_INVALID before anything is launched, mx_last_error naming the node.  mx_graph_adopt_state does not carry the setting. */
int mx_graph_set_video_source_matte(mx_graph* g, uint32_t node, const mx_video_matte_params* params /* NULL removes */);
/* The colour corrector as a per-source transform (mx_video_grade), under the keyer's rules: it applies to every frame the SOURCE_VIDEO node
 * delivers, whichever feeder brought it; a frame is graded once per setting and the result reused (a ring of n frames costs n launches, not one per tick); output frames
 * come from a pool and are rewritten only when the pool alone holds them.  The graph retains `lut`, so the caller may release it at once.  Where several transforms are set
 * on a node the order is GRADE, THEN KEY, THEN PLACE, whatever the call order: the input is corrected first and the key is decided on the corrected colour.  A scope tap on
 * the source's port sees the graded frame.  Setting it again drops what was cached under the old setting, from the next run on; params NULL removes the transform (lut is
 * then ignored).  MX_ERR_TYPE for a node that is not a SOURCE_VIDEO; MX_ERR_INVALID for a flag bit outside the three, a coefficient out of range, the LUT bit with no LUT
 * or a LUT without the bit, and together with mx_graph_set_video_source_band, in either call order (grading a band-scaled layer is a stated follow-up); each leaves the
 * graph usable.  A source frame that is not yuv420p / yuva420p fails the run with MX_ERR_INVALID before anything is launched, mx_last_error naming the node.
 * mx_graph_adopt_state does not carry the setting. */
int mx_graph_set_video_source_grade(mx_graph* g, uint32_t node, const mx_video_grade_params* params /* NULL removes */, mx_video_lut* lut);
/* One frame due on one tick of a SOURCE_VIDEO node: tick `tick` (absolute, as in mx_graph_run_ticks' first_tick + k) emits `frame` with the
 * given duration hint and tick offset; ticks without an entry emit None.  Entries are queued in ascending tick order, one per tick
 * (MX_ERR_INVALID otherwise), and while any is queued they take the place of mx_graph_set_video_source[_ring].  What
 * mx_media_source_feed / mx_stream_input_feed use; the graph retains the frame until its tick has run. */
int mx_graph_queue_video_source(mx_graph* g, uint32_t node, uint64_t tick, mx_dframe* frame, int64_t dur_num, int64_t dur_den,
                                int64_t off_num, int64_t off_den);

/* ---------------------------------------------------------------------------------------------- */
/* timed ingest: decoded frames with rational timestamps enter the engine  */
/* ---------------------------------------------------------------------------------------------- */

/* MediaSource::run_tick (src/module/media_source.rs:93-126): the decode thread sends (frame, pts, duration) over a channel of TWO
 * (sync_channel(2), :140); every tick takes at most one frame off the channel, moves its pts by the epoch -- the engine time of the
 * tick the FIRST frame was received on (:104-107) -- and emits the oldest buffered frame once its pts lies before the end of the tick
 * (:113-121), with tick_offset = pts - start of tick (negative for a late frame).  Timestamps are exact rationals in seconds
 * (util/src/time.rs:10-75); sample_rate / ticks_per_second 0 => 44100 / 60 (src/engine.rs:53-54). */
typedef struct mx_media_source mx_media_source;
int mx_media_source_create(uint32_t sample_rate, uint32_t ticks_per_second, mx_media_source** out);
void mx_media_source_destroy(mx_media_source* m);
/* MediaSourceEvent::SetMedia (:85-91): present = 1 installs a fresh OpenMedia (empty channel, no epoch, empty buffer, :140-147), 0 = None. */
int mx_media_source_set_media(mx_media_source* m, int present);
/* the decode thread's tx.send (:271): MX_ERR_FULL while two frames wait (the reference blocks), MX_ERR_INVALID without media (the
 * reference's thread ends, :272-276).  The source retains the frame.  Safe from another thread than the run_tick caller. */
int mx_media_source_send(mx_media_source* m, mx_dframe* frame, int64_t pts_num, int64_t pts_den, int64_t dur_num, int64_t dur_den);
/* One run_tick at engine time t (samples).  out->frame NULL = None; else it carries one reference for the caller. */
int mx_media_source_run_tick(mx_media_source* m, uint64_t t, mx_video_input* out);
/* n_ticks run_tick calls for ticks first_tick .. first_tick + n_ticks - 1, their frames queued on SOURCE_VIDEO `node`
 * (mx_graph_queue_video_source) for the mx_graph_run_ticks(first_tick, n_ticks) that follows. */
int mx_media_source_feed(mx_media_source* m, mx_graph* g, uint32_t node, uint64_t first_tick, uint32_t n_ticks);

/* StreamInput::run_tick (src/module/stream_input.rs:72-147) with both of its rings (src/source.rs:97-98, 65536 frames each): audio
 * frames (source id, source time, i16 samples of any length) are re-blocked to ticks exactly as mx_pcm_ring does; a frame from a source
 * id other than the one the tick started with re-bases the epoch = engine time - its source time (:100-106); the next video frame is due
 * at tick_offset = source time + epoch - engine time (< 0 or no source yet => 0, :127-133) and is held back while that lies beyond the
 * tick (:135-138). */
typedef struct mx_stream_input mx_stream_input;
int mx_stream_input_create(uint32_t sample_rate, mx_stream_input** out);
void mx_stream_input_destroy(mx_stream_input* s);
/* StreamInput::update with another mountpoint (:57-70): listening = 1 replaces both rings by empty ones, 0 leaves none (every write is
 * MX_ERR_FULL, every tick reads silence); the held frames and the source timing stay. */
int mx_stream_input_listen(mx_stream_input* s, int listening);
/* SourceSend::write_audio / write_video (src/source.rs:158-190); source_id != 0 (NonZeroUsize, :35).  MX_ERR_FULL = Err(()).
 * Safe from another thread than the run_tick caller. */
int mx_stream_input_write_audio(mx_stream_input* s, uint64_t source_id, int64_t ts_num, int64_t ts_den, const int16_t* interleaved, size_t n_samples);
int mx_stream_input_write_video(mx_stream_input* s, uint64_t source_id, int64_t ts_num, int64_t ts_den, mx_dframe* frame, int64_t dur_num, int64_t dur_den);
/* One run_tick at engine time t: audio_out[n_out] (n_out = 2 * SPT) receives the tick's interleaved i16 samples -- convert_sample's
 * input (:167-173) -- zero where the queue ran dry (*zero_filled samples); video_out as in mx_media_source_run_tick.  Host only. */
int mx_stream_input_run_tick(mx_stream_input* s, uint64_t t, int16_t* audio_out, size_t n_out, mx_video_input* video_out, size_t* zero_filled);
/* n_ticks run_tick calls: audio into SOURCE_STEREO `audio_node` (H2D as i16 from page-locked memory, / 32768 on the device), frames
 * queued on SOURCE_VIDEO `video_node` (UINT32_MAX = the video output is not connected). */
int mx_stream_input_feed(mx_stream_input* s, mx_graph* g, uint32_t audio_node, uint32_t video_node, uint64_t first_tick, uint32_t n_ticks,
                         size_t* zero_filled);

/* H2D staging ring for decoded frames (the reference moves frames between threads through rings, src/source.rs:97-98): `upload` packs the
 * host planes into the next page-locked slot, laid out like the device frame, and sends it as ONE asynchronous copy on the stager's own
 * stream; *out is a device frame (one reference for the caller) from a pool -- a frame nobody holds any more is written again, after
 * what the last fenced stream has queued.  A consumer stream must be fenced before it reads frames uploaded since the last fence.
 * A slot is reused only once its copy has completed (upload blocks until then): `slots` bounds the frames in flight. */
typedef struct mx_frame_stager mx_frame_stager;
int mx_frame_stager_create(uint32_t slots, mx_frame_stager** out);
void mx_frame_stager_destroy(mx_frame_stager* st);
int mx_frame_stager_upload(mx_frame_stager* st, const mx_frame* host, mx_pixfmt fmt, mx_dframe** out);
/* The copy-free form, for a decoder that can be given its picture buffers (AVCodecContext.get_buffer2): `acquire` hands out the plane
 * pointers and strides of a page-locked slot (rows 64-byte aligned, padding already blank), the decoder writes the picture there, `commit`
 * sends the slot as one asynchronous copy and returns the device frame.  Several slots may be held at once (reference pictures);
 * MX_ERR_FULL when all are.  A slot's memory is the caller's from acquire until commit. */
int mx_frame_stager_acquire(mx_frame_stager* st, uint32_t width, uint32_t height, mx_pixfmt fmt, mx_frame* host, uint32_t* ticket);
int mx_frame_stager_commit(mx_frame_stager* st, uint32_t ticket, mx_dframe** out);
int mx_frame_stager_fence(mx_frame_stager* st, void* stream);
int mx_frame_stager_fence_graph(mx_frame_stager* st, mx_graph* g);
int mx_frame_stager_sync(mx_frame_stager* st);

/* Output port of a video node after the last tick: one reference for the caller, NULL = None. */
int mx_graph_video_output(mx_graph* g, uint32_t node, uint32_t port, mx_dframe** out);
/* RGBA8 device buffer a VIDEO_TO_RGBA node wrote on the last tick (width/height 0 = no frame).  Written asynchronously on the graph's
 * stream: read it there, or after mx_graph_sync. */
int mx_graph_rgba_output(mx_graph* g, uint32_t node, void** device_rgba, int32_t* stride, uint32_t* width, uint32_t* height);

/* Video scope taps: taps on VIDEO output ports of a built graph -- what the meters and the spectrum taps are for the audio
 * half.  A tap observes a port: no module, no edge, the run order and the fusion plan unchanged; a graph without them launches nothing new
 * and its video path is unchanged call for call.  On every recorded tick each tap's frame is counted on the device, in one launch, into one
 * record.  BUILD-SPECIFIED (the reference has no scopes); every number is an integer count, so the records are fixed bit for bit whatever the
 * order of accumulation (tests/video_scope_model.py restates them in numpy):
 *   counted   a frame is counted when it is yuv420p or yuva420p (the coverage plane is ignored).  W x H is its visible luma size, the chroma
 *             planes are (W >> 1) x (H >> 1); stride padding is never counted.  All counts are uint32_t.
 *   hist      [3][256]: hist[0][v] = luma samples equal to v; hist[1], hist[2] the same for the U and V planes.  Minimum, maximum, mean and the
 *             legal-range violations (Y < 16, Y > 235, chroma outside 16 .. 240: crushed blacks, blown whites) are sums over these 768
 *             numbers, taken on the host: the record has NO fields for them.
 *   wave      [C][256], C = wave_cols (0: absent): wave[c][v] = luma samples of value v in column bucket c = floor(x * C / W), x the sample's
 *             column, in integer arithmetic -- the waveform monitor's picture.  x * C fits 32 bits for W <= 2^24 (C <= 256); frames are at
 *             most 16 384 wide.  A bucket without a column (W < C) stays 0.
 *   vec       [128][128], present when vectorscope != 0: vec[V >> 1][U >> 1] counts the (U, V) pairs of chroma samples at the same chroma position.
 *   record    per recorded tick and tap: a 32-byte header of uint32_t { present, counted, pixfmt, width, height, tick_in_run, reserved[2] },
 *             then hist, then wave, then vec: 32 + 4 * (768 + 256 * C + 16384 * [vectorscope != 0]) bytes (mx_video_scope_record_bytes).
 *             present = 0: the port held no frame that tick (Output = None, io.rs:76) -- everything but tick_in_run is 0.  A frame of another
 *             pixel format (the A / B outputs of a VideoMixer are clones of its inputs: packed RGB, nv12, deep YUV ...): present = 1,
 *             counted = 0, pixfmt (mx_pixfmt; MX_PIXFMT_YUVA420P for a yuv420p frame with a coverage plane) and the size filled, every count 0.
 *             No conversion is specified here: scopes of other formats are a follow-up.  reserved is 0.
 *   hop       >= 1.  The graph keeps ONE counter c: 0 when the taps are set, incremented once per video tick; a tick is recorded when
 *             c mod hop == 0 (tested before the increment); c is carried across runs.  A display wants 30 - 60 records a second, not one per
 *             tick of a 2048-tick run: with wave_cols = 256 and the vectorscope a record is 330 784 bytes.
 * One parameter set holds for every tap of the graph.  A frame that is still symbolic (an unevaluated cross-fade chain or scaler output) is
 * materialised on the graph's stream before it is counted: that write is the price of a tap; every picture the graph produces (composite,
 * RGBA sink, Monitor) is the same byte for byte with and without taps. */
typedef struct { uint32_t wave_cols /* 0, 64, 128 or 256 */, vectorscope /* 0: no vec */, hop /* >= 1 */; } mx_video_scope_params;
/* Replaces the graph's scope taps with ports[0..n) (n = 0: none; params may then be NULL and the graph launches nothing for them) and resets c.
 * Audio port: MX_ERR_TYPE.  A node or port out of range, a duplicate (node, port), wave_cols outside the list, hop = 0: MX_ERR_INVALID.
 * Device memory: ceil(max_ticks_per_run / hop) x n x record bytes for the last run's records; more than 4 GiB: MX_ERR_NOMEM (raise hop).
 * Waits for outstanding work like a read-back.  mx_graph_adopt_state does not carry taps: set them again on the new graph. */
int mx_graph_set_video_scopes(mx_graph* g, const mx_port_ref* ports, size_t n, const mx_video_scope_params* params);
/* The last run's records, [recorded tick][tap in set order], mx_video_scope_record_bytes each; *n_records = recorded ticks x taps (0 when no
 * tick of the run was recorded; dst may then be NULL).  cap_bytes smaller than that, no taps, or no run since they were set: MX_ERR_INVALID.
 * Joins the graph's streams like mx_graph_read_output. */
int mx_graph_read_video_scopes(mx_graph* g, void* dst, size_t cap_bytes, uint32_t* n_records);
/* Bytes of one record under `params` (hop is not looked at).  Host only: touches no device.  wave_cols outside the list: MX_ERR_INVALID. */
int mx_video_scope_record_bytes(const mx_video_scope_params* params, size_t* bytes);
/* The pixel-path form, beside mx_video_to_rgba: the record of ONE frame into device_record (4-byte aligned device memory of
 * mx_video_scope_record_bytes bytes), asynchronous on `stream`; present = 1, tick_in_run = 0, hop ignored. */
int mx_video_scope(const mx_dframe* in, const mx_video_scope_params* params, void* device_record, void* stream);

/* The multiviewer as a tap on VIDEO output ports (mx_video_multiview): view i shows the frame on ports[i] -- a SOURCE_VIDEO's port (keyed / placed
 * where such a transform is set: the placed canvas is what is shown) or a VideoMixer's program, A or B.  Like the video scope taps it adds no node and no edge: the run
 * order is unchanged and so is every picture the graph produces, byte for byte; a graph without the setting launches nothing new.  The same port may appear in several views.
 *   hop       the scopes' rule with a counter c of its own: c = 0 at the set, a tick is recorded when c mod hop == 0 (tested before the increment), c is carried across runs.
 *   render    a run renders AT MOST ONE canvas, that of its LAST recorded tick (earlier recorded ticks of the same run are not rendered: nobody could read them), at the
 *             end of that tick's pass over the video nodes.  A port whose frame is still symbolic (an unevaluated cross-fade chain or scaler output) is materialised first,
 *             as for a scope tap; then ONE launch follows on the graph's stream.  A port that holds no frame (None), or a frame of another pixel format, is a view not
 *             shown; present_mask still has its bit for the other format.
 *   status    recorded: how many ticks of the last run were recorded (0: none, and no canvas); tick_in_run: the rendered tick; present_mask: bit i, ports[i] held a frame
 *             on that tick; shown_mask: as mx_video_multiview.
 * mx_graph_set_multiview: n == params->n_views views; n = 0 (params may be NULL) removes the setting.  Audio port: MX_ERR_TYPE.  A node or port out of range,
 * n != n_views, hop = 0, or parameters mx_video_multiview refuses: MX_ERR_INVALID.  Waits for outstanding work like mx_graph_set_video_scopes and resets c.  The tap tables
 * are kept per view and rebuilt only when that view's source size or picture rectangle changes; per frame only the launch's small descriptor block is uploaded.
 * mx_graph_adopt_state does not carry the setting.
 * mx_graph_multiview_output: the canvas of the last run's last recorded tick, *out carrying one reference for the caller, and the status (may be NULL); recorded = 0 and
 * *out = NULL when the last run recorded no tick (no error).  No setting, or no run since it was set: MX_ERR_INVALID.  Joins the graph's streams like the other video
 * read-outs.  Canvases come from a small pool under the placer's rule: a pooled canvas is rewritten only when the pool alone holds it, so one the caller still holds is
 * never overwritten. */
typedef struct { uint32_t recorded, tick_in_run, present_mask, shown_mask; } mx_multiview_status;   /* 16 bytes */
int mx_graph_set_multiview(mx_graph* g, const mx_port_ref* ports, size_t n, const mx_multiview_params* params);   /* n == params->n_views; n = 0 (params may be NULL) removes */
int mx_graph_multiview_output(mx_graph* g, mx_dframe** out, mx_multiview_status* status);

/* MX_KIND_MONITOR after a run.  Tick `tick_in_run` of the last mx_graph_run_ticks as the codec thread would see it:
 * ts = the tick's timestamp relative to the node's epoch -- the first tick it ever ran (monitor.rs:121-123); when the Video input carried
 * a frame: *frame = that picture through the node's DynamicScaler (the input itself when it already has the encoder's size,
 * encode.rs:342-345; one reference for the caller, still on the device: download it or hand it to a device encoder), frame_ts = ts +
 * tick_offset (monitor.rs:229), dur = its duration hint; else video_present = 0 and *frame = NULL.  The reference DROPS a tick when its
 * codec thread lags (try_send on a channel of two, monitor.rs:163-177): a node built with mx_monitor_params_ex.queue_depth > 0 does the same
 * (`dropped`, below: nothing is scaled for such a tick, until mx_graph_monitor_consume frees slots); the short parameter form keeps every tick.
 * Device memory inside a batched run (MX_VIDEO_BATCH = K ticks per launch, default 16): every scaled layer's Scaler holds a ring of 2K output
 * frames (1080p yuv420p: 32 x 3.1 MB = 100 MB per scaled layer) and every VIDEO_TO_RGBA node K RGBA buffers (16 x 8.3 MB = 133 MB). */
typedef struct { int32_t video_present; int64_t ts_num, ts_den, frame_ts_num, frame_ts_den, dur_num, dur_den;
                 int32_t dropped; /* mx_monitor_params_ex.queue_depth > 0: the queue was full, the codec thread never gets this tick (nor its audio) */ int32_t _pad; } mx_monitor_tick;
int mx_graph_read_monitor_tick(mx_graph* g, uint32_t node, uint32_t tick_in_run, mx_monitor_tick* info, mx_dframe** frame);
/* queue_depth > 0: the consumer (the codec thread's rx.recv, monitor.rs:226) has taken n_ticks ticks off the node's queue: that many slots are free
 * for the ticks of the next submissions.  More than are queued empties the queue. */
int mx_graph_monitor_consume(mx_graph* g, uint32_t node, uint32_t n_ticks);
/* All kept pictures of ticks [first_tick, first_tick + n_ticks) of the last run in ONE read-back: one gather launch on the device, one
 * D2H copy.  frames[n_ticks * frame_bytes]: slot k holds tick first_tick + k's picture in the layout mx_graph_monitor_layout reports (rows
 * 64-byte aligned: an AVFrame.linesize an encoder takes as is); present[k] = 0 leaves slot k untouched.  A page-locked `frames` avoids
 * the runtime's staging copy. */
typedef struct { uint32_t width, height; size_t frame_bytes; size_t plane_offset[3]; int32_t stride[3]; } mx_monitor_layout;
int mx_graph_monitor_layout(mx_graph* g, uint32_t node, mx_monitor_layout* out);
int mx_graph_read_monitor_video(mx_graph* g, uint32_t node, uint32_t first_tick, uint32_t n_ticks, uint8_t* frames, uint8_t* present);
/* The mix the node received over the first n_ticks ticks of the last run, as the encoder's PCM: clamp to [-1, 1], * 32767, truncate
 * (encode.rs:183-195), converted on the device: audio[n_ticks * 2 * SPT].  A Disconnected input reads zeros (io.rs:56-57). */
int mx_graph_read_monitor_audio_i16(mx_graph* g, uint32_t node, int16_t* audio, uint32_t n_ticks);

/* ---------------------------------------------------------------------------------------------- */
/* multi-GPU: the bus exchange of a strip-sharded job                       */
/* ---------------------------------------------------------------------------------------------- */

/* One process per GPU, the reference's single engine thread (src/engine.rs:78-96) in each.  Strips are partitioned contiguously
 * over the ranks; the sharded job is DEFINED as the reference-expressible graph  N x Mixer(strips / N) -> Mixer(N, unity gains):
 * every sample of the whole Master / Cue bus is the f32 sum of the N partial buses in rank order 0 .. N-1 (Mixer::run_tick,
 * src/module/mixer.rs:57-68, applied to the partials), and every rank ends with it.  The exchange runs on its own stream,
 * pipelined against the next step's compute: two steps may be in flight.
 *   MX_EXCHANGE_ALLGATHER  one ncclAllGather of the [master | cue] partials, then the rank-ordered sum: (N - 1) bus lengths received
 *   MX_EXCHANGE_SLICES     ordered reduce-scatter + all-gather: the step's ticks are cut into N time slices, rank j receives slice j
 *                          of every partial (grouped ncclSend / ncclRecv), sums it in rank order, an all-gather distributes the
 *                          finished slices: 2 (N - 1) / N bus lengths received.  Bit-identical to ALLGATHER.  n_ticks % N == 0.
 *   MX_EXCHANGE_ALLREDUCE  ncclAllReduce(sum): NOT the summation order of any graph the reference can express (non-parity mode)
 *   MX_EXCHANGE_AUTO       SLICES when N >= 4 and the ticks divide, else ALLGATHER */
enum { MX_EXCHANGE_AUTO = 0, MX_EXCHANGE_ALLGATHER = 1, MX_EXCHANGE_SLICES = 2, MX_EXCHANGE_ALLREDUCE = 3 };
#define MX_EXCHANGE_ID_BYTES 128   /* sizeof(ncclUniqueId) */
typedef struct mx_exchange mx_exchange;
typedef struct mx_loopback_group mx_loopback_group;

/* ncclGetUniqueId: rank 0 makes the job's id and hands the 128 bytes to the other ranks by any means it has (the reference's
 * hosts already talk over sockets); every rank passes them to mx_exchange_create, which is collective (ncclCommInitRank).
 * librccl is bound on first use (dlopen of librccl.so.1): a host without it still loads this library and gets MX_ERR_DEVICE here.
 * MX_RCCL_LIB (environment) names another library to bind in its place -- the test suite's stand-in for RCCL between processes that
 * share one GPU (tests/helpers/fake_rccl.c), through which the RCCL transport's own code runs with 2 and 4 real peers on a one-GPU box. */
int mx_exchange_unique_id(void* id_out /* MX_EXCHANGE_ID_BYTES */);
/* In-process transport for `world` exchanges of ONE process (virtual ranks on one GPU, or one thread driving several GPUs):
 * device-to-device copies stand in for the collectives; buffers, combine and pipelining are the RCCL path's.  Every member
 * submits step k before any member submits step k + 1.  Destroy the group after its exchanges. */
int mx_loopback_group_create(uint32_t world, mx_loopback_group** out);
void mx_loopback_group_destroy(mx_loopback_group* grp);

/* Exchange of Mixer `mixer_node`'s two output buses of `g` over steps of `n_ticks` ticks (<= max_ticks_per_run).  Exactly one of
 * nccl_unique_id / loopback is given.  `g` must outlive the exchange.  Over a graph whose Mixer bank runs on the second stream (MX_FLAG_OVERLAP_TAIL or the automatic mode,
 * which an exchange does NOT end) an RCCL exchange's pack and collectives of step k go out behind the bank when the graph releases it -- with run k + 1, or when the step's
 * result is asked for (wait / result / read_result / elapsed_ms / sync) -- and run k + 2 starts after them; the loopback transport joins the streams at the submit. */
int mx_exchange_create(mx_graph* g, uint32_t mixer_node, uint32_t n_ticks, uint32_t rank, uint32_t world,
                       const void* nccl_unique_id, mx_loopback_group* loopback, uint32_t mode, mx_exchange** out);
void mx_exchange_destroy(mx_exchange* x);
/* After mx_graph_run_ticks of step `step` (any increasing numbering): pack the partial buses on the graph's stream and queue the
 * exchange + combine behind them on the exchange's stream.  Asynchronous.  Steps `step` and `step - 1` stay readable. */
int mx_exchange_submit(mx_exchange* x, uint64_t step);
/* Make `stream` (NULL = the graph's stream) wait for step `step`'s combined bus. */
int mx_exchange_wait(mx_exchange* x, uint64_t step, void* stream);
/* Device pointers of the combined Master / Cue of step `step` (n_ticks tick buffers each, interleaved stereo): valid on a stream
 * that waited (mx_exchange_wait), until step + 2 is submitted -- or, when the consumer reads them on a stream of its own, until
 * the point it marks with mx_exchange_release (the exchange orders its next write of those buffers after that point). */
int mx_exchange_result(mx_exchange* x, uint64_t step, void** master_device, void** cue_device, size_t* floats_per_bus);
int mx_exchange_release(mx_exchange* x, uint64_t step, void* stream);
/* The same to host memory, synchronously (either pointer may be NULL). */
int mx_exchange_read_result(mx_exchange* x, uint64_t step, float* master, float* cue);
/* Device time of step `step`'s exchange on its own stream (collectives + combine), ms; waits for it. */
int mx_exchange_elapsed_ms(mx_exchange* x, uint64_t step, float* ms);
int mx_exchange_sync(mx_exchange* x);
typedef struct { uint32_t mode, rank, world, loopback; uint64_t floats_per_bus, bytes_received_per_step; } mx_exchange_info;
int mx_exchange_get_info(const mx_exchange* x, mx_exchange_info* out);

/* plain device memory for consumers of mx_video_to_rgba (tests, bench) */
int mx_device_alloc(size_t bytes, void** device_ptr);
void mx_device_free(void* device_ptr);
int mx_device_download(void* host, const void* device_ptr, size_t bytes, void* stream);   /* synchronous */
/* page-locked host memory for the buffers that cross PCIe every submission (mx_graph_read_monitor_video's `frames`, PCM, sources):
 * copies from / to it are one DMA, without the runtime's staging through its own pinned bounce buffers */
int mx_host_alloc(size_t bytes, void** host_ptr);
void mx_host_free(void* host_ptr);

/* ---- per-module compatibility path: one ModuleT instance, host pointers in and out ---- */

typedef struct { mx_line kind; const float* samples; size_t len; const mx_frame* video; } mx_input;                 /* InputRef, io.rs:19-24 */
typedef struct { mx_line kind; float* samples; size_t len; mx_frame* video; int video_present; } mx_output;         /* OutputRef, io.rs:96-100 */

typedef struct mx_module mx_module;

/* ModuleT::create (src/module/mod.rs:12) at the reference's compile-time 44100 Hz / 60 ticks. */
int mx_module_create(uint32_t kind, const void* params, size_t params_len, mx_module** out);
/* Same with explicit rates/flags (only sample_rate, ticks_per_second, flags, device are read). */
int mx_module_create_ex(uint32_t kind, const void* params, size_t params_len, const mx_graph_opts* opts, mx_module** out);
/* ModuleT::update */
int mx_module_update(mx_module* m, const void* params, size_t params_len);
/* ModuleT::run_tick (src/module/mod.rs:17): inputs/outputs are host buffers owned by the caller
 * for the duration of the call; outputs are fully overwritten.  A MX_DISCONNECTED input reads the
 * zero buffer.  Any input length is accepted (the reference's one test feeds 355 285 samples in
 * one call, src/module/eq_three.rs:150-167) as long as all ports agree.  Plotter: *indication_len is IN/OUT --
 * on entry the capacity of `indication` in bytes, on return the bytes written (0 = None): left[frames] then
 * right[frames] f32 for the call's buffer length; a capacity below 2 * frames floats is MX_ERR_INVALID.
 * EqThree always runs in the reference's exact order on this path unless MX_FLAG_EQ_FAST was given at creation. */
int mx_module_run_tick(mx_module* m, uint64_t t, const mx_input* inputs, size_t n_inputs,
                       mx_output* outputs, size_t n_outputs, void* indication, size_t* indication_len);
void mx_module_destroy(mx_module* m);

#ifdef __cplusplus
}
#endif
#endif /* MIXLAB_GPU_H */

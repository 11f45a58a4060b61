// mx_video_graph.hpp -- what the engine keeps per video node and per video tap, out of Graph and Node: the state of a SOURCE_VIDEO (with the colour corrector, the keyer,
// the matte refiner and the placer as its SourceTransform), of a VIDEO_TO_RGBA sink and of a MONITOR, and the two taps on video ports -- the scope taps and the multiviewer.  Graph
// (mx_engine.hpp) walks the video nodes tick by tick and calls in here; the taps see it through TapHost (mx_taps.hpp), like the audio tap sets.
#pragma once
#include <deque>
#include <memory>
#include <vector>

#include "mx_common.hpp"
#include "mx_taps.hpp"
#include "mx_video.hpp"

namespace mx {

struct VOut { FrameRef frame; Rational dur, off; };   // a video output terminal's frame of the tick being run (empty FrameRef = None)

// The taps' hop rule, once: the counter is 0 when the taps are set, +1 per video tick, carried across runs; a tick is recorded when the counter is a
// multiple of the hop BEFORE the increment.
struct HopCounter {
    uint64_t hop = 1, c = 0;
    void reset(uint64_t hop_ = 1) { hop = hop_; c = 0; }
    struct Run { uint64_t first, count; };   // the first recorded tick of a run (counted from the run's first) and how many it records
    Run begin_run(uint64_t n_calls) const { const uint64_t first = (hop - c % hop) % hop; return Run{first, first < n_calls ? (n_calls - first + hop - 1) / hop : 0}; }
    bool tick() { return c++ % hop == 0; }   // record this tick?  Then advance
};

// The colour corrector, the keyer, the matte refiner and the placer as a transform of a SOURCE_VIDEO's frames (mx_graph_set_video_source_grade / _key / _matte /
// _place): grade, then key, then matte, then place, where several are set.  A frame is transformed once per setting.
class SourceTransform {
public:
    void set_grade(const mx_video_grade_params* p, std::shared_ptr<const LutTables> lut);   // nullptr removes; the parameters were checked
    void set_key(const mx_video_key_params* p);       // nullptr removes; the parameters were checked
    void set_matte(const mx_video_matte_params* p);   // likewise
    void set_place(const mx_video_place_params* p);   // likewise
    bool grade_on() const { return grade_on_; }
    bool key_on() const { return key_on_; }
    bool matte_on() const { return matte_on_; }
    bool place_on() const { return place_on_; }
    bool active() const { return grade_on_ || key_on_ || matte_on_ || place_on_; }
    const char* input_error(const DFrame* f) const;   // nullptr, or why the transform cannot take this frame
    FrameRef apply(const FrameRef& src, hipStream_t s);
private:
    // Frames transformed under the current setting, newest last: an entry holds the source frame (so its address stays its identity) and lives while anything
    // else does.  With several stages set, src is the frame the FEEDER delivered and out the LAST stage's frame: a graded, keyed or matted frame between two passes is a
    // pool frame nobody else sees, read by the pass launched right behind it on the stream, and is listed nowhere.
    struct DoneCache {
        struct Entry { FrameRef src, out; };
        std::vector<Entry> list;
        FrameRef find(const DFrame* src) const { for (const Entry& e : list) if (e.src.f == src) return e.out; return FrameRef(); }
        void make_room();   // entries whose source frame only this list still holds can never be asked for again; the oldest goes too when the list is full (32)
        void clear() { list.clear(); }
    };
    bool grade_on_ = false, key_on_ = false, matte_on_ = false, place_on_ = false;
    mx_video_grade_params grade_{};
    std::shared_ptr<const LutTables> grade_lut_;      // retained for as long as the setting stands: the caller may release its handle at once
    mx_video_key_params key_{};
    mx_video_matte_params matte_{};
    mx_video_place_params place_{};
    std::shared_ptr<const PlaceTables> place_tabs_;   // of the current setting (and, for a whole-frame crop, of the size of the frame seen last)
    DoneCache graded_, keyed_, matted_, placed_;   // the list of the LAST stage set is the one in use: placed_, else matted_, else keyed_, else graded_
    void clear_done() { graded_.clear(); keyed_.clear(); matted_.clear(); placed_.clear(); }
    // output frames.  64 is twice the list above: a frame that leaves the list is still in the pool, so a long ring recycles frames instead of allocating
    FramePool grade_pool_{64}, key_pool_{64}, matte_pool_{64}, place_pool_{64};
};

struct VideoSourceState {   // SOURCE_VIDEO
    FrameRef frame; Rational dur, off; bool repeat = false, pending = false;   // the set frame (mx_graph_set_video_source); dur / off are the ring's too
    std::vector<FrameRef> ring; size_t ring_pos = 0;                           // a new frame every tick, cycling
    struct Sched { uint64_t tick; FrameRef frame; Rational dur, off; };
    std::deque<Sched> sched;                                                   // frames due on given ticks (MediaSource / StreamInput pacing), oldest first
    // frames are halo slices, delivered as this rank's row band of the scaled picture.  The pool matches on nothing: every frame in it is full_w x band_rows of
    // the one BandScaler, and set_video_source_band clears it with the scaler
    std::shared_ptr<BandScaler> band; FramePool band_pool{8};
    SourceTransform transform;

    VOut due(uint64_t tick, hipStream_t s);   // the frame due on `tick`: queue, then ring, then set frame; banded, then transformed
    // every frame a run over ticks [tick0, last] may deliver, before any of it has run
    template <class Look> void each_deliverable(uint64_t tick0, uint64_t last, Look look) const {
        for (const Sched& e : sched) if (e.tick >= tick0 && e.tick <= last) look(e.frame.f);
        if (sched.empty() || sched.back().tick < last) {   // ticks of the run past the queue fall through to the ring / the set frame
            if (!ring.empty()) { for (const FrameRef& f : ring) look(f.f); }
            else if (frame && (repeat || pending)) look(frame.f);
        }
    }
    void adopt(const VideoSourceState& old);   // what crosses a topology edit
};

struct RgbaSinkState {   // VIDEO_TO_RGBA
    std::vector<DevBuf> buf; uint32_t cur = 0, w = 0, h = 0; int32_t stride = 0;   // video_batch_ticks() buffers, written in turn (that many ticks' chains may share a launch); cur = the last tick's
    struct Pending { ChainRgbaArgs args; std::shared_ptr<LazyChain> keep; };
    std::vector<Pending> pending;   // chains of the last ticks, not launched yet, oldest first
    uint32_t calls = 0;             // sink calls that queued a chain in this run
    void run_tick(const VOut* in, const mx_video_to_rgba_params& p, TapHost& host);   // in: nullptr = Disconnected
    void launch_pending(size_t count, bool with_queued_scales, hipStream_t s);        // the `count` oldest pending chains
    void end_run(hipStream_t s) { if (!pending.empty()) launch_pending(pending.size(), false, s); calls = 0; }   // the last ticks' chains
};

struct MonitorState {   // MONITOR: what the sink kept of every tick of the last run
    struct Tick { bool present = false, dropped = false; FrameRef frame; Rational ts, frame_ts, dur; };
    struct Layout { uint32_t width, height; size_t frame_bytes, plane_offset[3]; uint32_t stride[3]; };
    bool has_epoch = false; Rational epoch;
    uint32_t depth = 0, queued = 0;   // mx_monitor_params_ex.queue_depth (0 = keep every tick) and the ticks the consumer has not taken yet
    std::vector<Tick> ticks;
    std::shared_ptr<Scaler> scaler;
    DevBuf pack;                      // the packed read-back's device staging
    void run_tick(Rational absolute, const VOut* in);   // in: nullptr = Disconnected
    Layout layout() const;            // of every kept frame
};

// Video scope taps (mx_graph_set_video_scopes / mx_graph_read_video_scopes): histograms, waveform and vectorscope of the frames on video ports.  The taps in
// set order; rec_: the last run's records [recorded tick][tap], cap_ ticks of room.
class VideoScopeTaps {
public:
    explicit VideoScopeTaps(TapHost& host) : host_(host) {}
    void set(const mx_port_ref* ports, size_t n, const mx_video_scope_params* params);
    void begin_run(uint32_t n_calls);   // the records this run will count into are cleared, in one fill on the stream ahead of every launch of the run
    void empty_run() { n_rec_ = 0; }
    void begin_tick(uint32_t tick_in_run) { now_ = !ports_.empty() && hop_.tick(); tick_in_run_ = tick_in_run; }
    void node_ran(uint32_t id) { if (now_) for (uint32_t k = 0; k < (uint32_t)ports_.size(); ++k) if (ports_[k].node == id) launch(k); }   // its outputs are set, nothing downstream has run
    void end_tick() { if (now_) ++n_rec_; }
    size_t read(void* dst, size_t cap_bytes);   // the last run's records; returns how many
private:
    void launch(uint32_t tap);
    TapHost& host_;
    std::vector<mx_port_ref> ports_;
    mx_video_scope_params par_{0, 0, 1};
    size_t rec_bytes_ = 0, cap_ = 0;
    DevBuf rec_;
    HopCounter hop_;
    uint32_t n_rec_ = 0;          // recorded ticks of the run in progress / of the last run
    uint32_t tick_in_run_ = 0;    // the tick being run, counted from the run's first
    bool now_ = false, run_seen_ = false;   // the tick being run is recorded; a run was made since the taps were set
};

// The multiviewer as a tap on video ports (mx_graph_set_multiview / mx_graph_multiview_output): the ports' frames, in view order, tiled on one canvas.  Its
// own hop counter, the scopes' rule.  A run renders ONE canvas, at the end of the last tick of the run its counter records.
class MultiviewTap {
public:
    explicit MultiviewTap(TapHost& host) : host_(host) {}
    void set(const mx_port_ref* ports, size_t n, const mx_multiview_params* params);   // n = 0 removes
    void clear() { out_ = FrameRef(); pool_.clear(); }
    void begin_run(uint32_t n_calls);   // which tick the run renders follows from the counter now
    void empty_run() { out_ = FrameRef(); status_ = mx_multiview_status{0, 0, 0, 0}; }
    void begin_tick() { now_ = !ports_.empty() && hop_.tick(); }
    void end_tick(uint32_t tick_in_run) { if (now_ && (int64_t)tick_in_run == last_) render(tick_in_run); }   // every tapped port's frame is set
    FrameRef output(mx_multiview_status* status);   // the canvas of the last run's last recorded tick (null: none recorded)
private:
    void render(uint32_t tick_in_run);
    TapHost& host_;
    std::vector<mx_port_ref> ports_;
    mx_multiview_params par_{};
    MultiviewTabs tabs_;
    FramePool pool_{8};   // canvases.  Matches on nothing: every frame in it has the canvas size of the current setting, and every set() clears it
    FrameRef out_;
    mx_multiview_status status_{0, 0, 0, 0};
    HopCounter hop_;
    int64_t last_ = -1;   // the tick the run in progress renders (-1: none)
    bool now_ = false, run_seen_ = false;
};

}  // namespace mx

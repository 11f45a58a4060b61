// mx_video_graph.cpp -- per-node video state, the source transform, the taps on video ports (mx_video_graph.hpp), and the video section of Graph: the
// tick-by-tick walk over the video nodes and what the ABI sets and reads of them.
#include "mx_engine.hpp"

#include <algorithm>
#include <cstring>

namespace mx {

// ---- SOURCE_VIDEO ----
void SourceTransform::DoneCache::make_room() {
    for (size_t i = 0; i < list.size();) {
        if (list[i].src->rc.load(std::memory_order_acquire) == 1) list.erase(list.begin() + (ptrdiff_t)i); else ++i;
    }
    if (list.size() >= 32) list.erase(list.begin());
}

void SourceTransform::set_grade(const mx_video_grade_params* p, std::shared_ptr<const LutTables> lut) {
    // frames graded under the old setting are of no use, and neither is what was keyed or placed from them; the output frames stay in the pool (they match on size
    // and coverage, not on the setting) and are rewritten once their last holder has let go.  The old lattice lives until the launches that read it are behind the
    // new setting's on the stream: hipFree waits for the device
    clear_done();
    grade_on_ = p != nullptr;
    if (p) { grade_ = *p; grade_lut_ = std::move(lut); } else { grade_lut_.reset(); grade_pool_.clear(); }
}

void SourceTransform::set_key(const mx_video_key_params* p) {
    // frames keyed under the old setting are of no use; their output frames stay in the pool and are rewritten once their last holder has let go
    keyed_.clear();
    matted_.clear(); placed_.clear();   // a matted or placed frame holds the picture as it was keyed
    graded_.clear();   // listed only while the grade is the last stage: entries from before must not pin their pool frames
    key_on_ = p != nullptr;
    if (p) key_ = *p; else key_pool_.clear();
}

void SourceTransform::set_matte(const mx_video_matte_params* p) {
    // as for the key: frames refined under the old setting are of no use, nor what was placed from them; the lists of the stages ahead are in use only while theirs
    // is the last stage, and entries from before must not pin their pool frames.  The output frames stay in the pool and are rewritten once their last holder has let go
    clear_done();
    matte_on_ = p != nullptr;
    if (p) matte_ = *p; else matte_pool_.clear();
}

void SourceTransform::set_place(const mx_video_place_params* p) {
    // as for the key: frames placed under the old setting are of no use; a canvas of another size needs other frames, so the pool goes too
    placed_.clear(); place_pool_.clear(); place_tabs_.reset();
    place_on_ = p != nullptr;
    if (p) place_ = *p;
    keyed_.clear();   // the keyed frames a placed source needs are the placer's alone and never listed; those listed before must not pin their pool frames
    graded_.clear(); matted_.clear();  // likewise
}

const char* SourceTransform::input_error(const DFrame* f) const {
    if (grade_on_ && !key_input_ok(f)) return "the colour corrector takes yuv420p or yuva420p frames (mx_graph_set_video_source_grade)";
    if (key_on_ && !key_input_ok(f)) return "the keyer takes yuv420p or yuva420p frames (mx_graph_set_video_source_key)";
    if (matte_on_ && !key_input_ok(f)) return "the matte refiner takes yuv420p or yuva420p frames (mx_graph_set_video_source_matte)";
    return place_on_ ? place_input_error(f, place_) : nullptr;   // the grade, the key and the matte keep the frame's size, so the crop is checked against the frame as it arrives
}

// `src` graded (where a grade is set), then keyed (where a key is), then matted (where a matte is), then placed (where a placement is): once per setting, reused while anything but the list holds
// the source frame.
FrameRef SourceTransform::apply(const FrameRef& src, hipStream_t s) {
    // Graph::run looked at every frame the run can deliver before it launched anything
    if (input_error(src.f)) throw Error(MX_ERR_INTERNAL, "a video source's transform met a frame the run's check of its frames did not see");
    DoneCache& done = place_on_ ? placed_ : (matte_on_ ? matted_ : (key_on_ ? keyed_ : graded_));
    if (FrameRef o = done.find(src.f)) return o;
    done.make_room();
    FrameRef o = src;
    if (grade_on_) {   // the pools match on the size (and this one on the coverage plane): the frames have the source frames' sizes, which may differ from one to the next
        const uint32_t w = src->width, h = src->height;
        const bool al = src->with_alpha;
        o = grade_pool_.take([&](const DFrame& f) { return f.width == w && f.height == h && f.with_alpha == al; },
                             [&] { return DFrame::create(w, h, s, MX_PIXFMT_YUV420P, al); });   // the corrector leaves the padding as DFrame::create made it
        grade_into(src.f, grade_, grade_lut_.get(), o.f, s);
    }
    if (key_on_) {
        const FrameRef in = o;
        const uint32_t w = src->width, h = src->height;
        o = key_pool_.take([&](const DFrame& f) { return f.width == w && f.height == h; },
                           [&] { return DFrame::create(w, h, s, MX_PIXFMT_YUV420P, true); });   // the keyer leaves the padding as DFrame::create made it
        key_into(in.f, key_, o.f, s);
    }
    if (matte_on_) {   // refines what the key decided (or the coverage the frame came with); the placer resamples the refined plane
        const FrameRef in = o;
        const uint32_t w = src->width, h = src->height;
        o = matte_pool_.take([&](const DFrame& f) { return f.width == w && f.height == h; },
                             [&] { return DFrame::create(w, h, s, MX_PIXFMT_YUV420P, true); });   // the refiner leaves the padding as DFrame::create made it
        matte_into(in.f, matte_, o.f, s);
    }
    if (place_on_) {
        const FrameRef in = o;
        if (!place_tabs_ || !place_tables_fit(*place_tabs_, in.f, place_)) place_tabs_ = make_place_tables(in.f, place_);
        const uint32_t w = place_.canvas_w, h = place_.canvas_h;
        o = place_pool_.take([&](const DFrame& f) { return f.width == w && f.height == h; },
                             [&] { return DFrame::create_unfilled(w, h, MX_PIXFMT_YUV420P, true); });   // the placer writes every byte
        place_into(in.f, place_, *place_tabs_, o.f, s);
    }
    done.list.push_back(DoneCache::Entry{src, o});
    return o;
}

VOut VideoSourceState::due(uint64_t tick, hipStream_t s) {
    VOut v;   // None unless a frame is due
    while (!sched.empty() && sched.front().tick < tick) sched.pop_front();   // a tick that was never run
    if (!sched.empty()) {   // paced ingest: the tick a MediaSource / StreamInput emitted the frame on, or None
        if (sched.front().tick == tick) {
            Sched& e = sched.front();
            v = VOut{e.frame, e.dur, e.off};
            sched.pop_front();
        }
    } else if (!ring.empty()) {   // a decoder's stream: the next frame of the ring, every tick
        v = VOut{ring[ring_pos], dur, off};
        ring_pos = (ring_pos + 1) % ring.size();
    } else if (frame && (repeat || pending)) {
        v = VOut{frame, dur, off};
        pending = false;
    }
    if (band && v.frame) {   // row-band sharding: the frame is a halo slice of a smaller layer; deliver this rank's band of its scale
        FrameRef o = band_pool.take([](const DFrame&) { return true; }, [&] { return DFrame::create(band->full_w(), band->band_rows(), s); });
        band->run(v.frame.f, o.f, s);
        v.frame = o;
    }
    if (transform.active() && v.frame) v.frame = transform.apply(v.frame, s);
    return v;
}

void VideoSourceState::adopt(const VideoSourceState& old) {
    ring = old.ring; ring_pos = old.ring_pos;
    sched = old.sched;
    band = old.band; band_pool = old.band_pool;
    frame = old.frame; dur = old.dur; off = old.off; repeat = old.repeat; pending = old.pending;
    // `transform` is NOT carried: mixlab_gpu.h says of mx_graph_set_video_source_grade, of _key, of _matte and of _place "mx_graph_adopt_state does not carry the setting"
}

// ---- VIDEO_TO_RGBA ----
void RgbaSinkState::run_tick(const VOut* in, const mx_video_to_rgba_params& p, TapHost& host) {
    const hipStream_t s = host.stream();
    auto let_go = [&] { if (!pending.empty()) { flush_scales(s); launch_pending(pending.size(), false, s); } };   // with whatever scales are queued
    w = h = 0;
    if (!in || !in->frame) { let_go(); return; }   // no picture this tick: nothing will follow the pending chains soon
    DFrame* d = in->frame.f;
    const int32_t row = (int32_t)(((size_t)d->width * 4 + 15) & ~(size_t)15);
    const size_t need = (size_t)row * d->height;
    const uint32_t K = video_batch_ticks();   // ticks whose chains share one launch inside a batched run
    if (buf.size() != K || buf[0].bytes < need) {
        let_go();
        host.sync();
        buf.clear(); buf.resize(K);
        for (DevBuf& b : buf) b.alloc(need);
        cur = 0;
    }
    cur = (cur + 1u) % K;
    uint8_t* const out = (uint8_t*)buf[cur].p;
    if (d->lazy) {   // the composite only exists as a cross-fade chain: evaluate it straight into RGBA
        ChainRgbaArgs c{};
        fill_chain_rgba_sources(*d->lazy, c, s);   // layers that are unevaluated scaler outputs are resampled inside the kernel
        c.rgba = out; c.rgba_stride = (uint32_t)row; c.width = d->width; c.height = d->height;
        c.use_matrix = p.use_matrix;
        for (int k = 0; k < 12; ++k) c.m[k] = p.matrix_q12[k];
        // Inside a batched run the sink runs LATE and K ticks at a time (K = video_batch_ticks(), default 16): the chains of ticks k .. k + K - 1
        // leave in ONE launch together with the scaler tiles ticks k + K .. k + 2K - 1 queued (mx_k_video.hip k_video_batch) -- the
        // chip then holds waves of several frames in every phase at once instead of marching through load / compute / store in step.
        // Every K-th sink call is an event: it takes ALL queued scales along (so the scales a chain needs left at its own event
        // or an earlier one) and, once 2K chains are pending, the K oldest -- always at least K calls old.  A Scaler writes 2K output
        // frames in turn and the sink K RGBA buffers, so nothing in one launch writes what something else in it reads or writes.
        // What is still pending when the run ends is launched then.
        pending.push_back(Pending{c, d->lazy});
        if ((++calls % K) == 0) {
            if (pending.size() >= 2 * (size_t)K) launch_pending(K, true, s);
            else flush_scales(s);
        }
        w = d->width; h = d->height; stride = row;
        return;
    }
    let_go();
    d->ensure_pixels(s);
    if (d->fmt != MX_PIXFMT_YUV420P) throw Error(MX_ERR_INVALID, "VIDEO_TO_RGBA takes yuv420p (a VideoMixer output); put a VideoMixer in front of a source of another format");
    RgbaArgs a;
    a.y = d->data[0]; a.u = d->data[1]; a.v = d->data[2]; a.rgba = out;
    a.y_stride = d->stride[0]; a.u_stride = d->stride[1]; a.v_stride = d->stride[2]; a.rgba_stride = (uint32_t)row;
    a.width = d->width; a.height = d->height; a.use_matrix = p.use_matrix;
    for (int k = 0; k < 12; ++k) a.m[k] = p.matrix_q12[k];
    launch_yuv420_to_rgba(a, s);
    w = d->width; h = d->height; stride = row;
}

void RgbaSinkState::launch_pending(size_t count, bool with_queued_scales, hipStream_t s) {
    count = std::min(count, pending.size());
    const size_t K = std::min<size_t>(video_batch_ticks(), MX_VB_MAX_CHAINS);   // the sink's K RGBA buffers are written in turn: at most K chains per launch
    std::vector<ChainRgbaArgs> c(K);
    size_t i = 0;
    while (i < count) {
        const int m = (int)std::min(K, count - i);
        for (int k = 0; k < m; ++k) c[k] = pending[i + k].args;
        if (with_queued_scales && i == 0) launch_chains_rgba_after_queued_scales(c.data(), m, s);
        else launch_video_batch(nullptr, 0, c.data(), m, s);
        i += m;
    }
    pending.erase(pending.begin(), pending.begin() + count);
}

// ---- MONITOR ----
// Monitor::run_tick (monitor.rs:113-139) + the codec thread's use of the Tick (monitor.rs:226-236)
void MonitorState::run_tick(Rational absolute, const VOut* in) {
    Tick mt;
    if (!has_epoch) { epoch = absolute; has_epoch = true; }   // epoch.get_or_insert
    mt.ts = absolute - epoch;                                   // remove_epoch
    if (depth && queued >= depth) {                             // try_send on a full channel: the tick is dropped (monitor.rs:163-177)
        mt.dropped = true;
        ticks.push_back(std::move(mt));
        return;
    }
    if (depth) ++queued;
    if (in && in->frame) {
        mt.present = true;
        mt.frame_ts = mt.ts + in->off;                          // tick.timestamp + tick_offset
        mt.dur = in->dur;
        mt.frame = scaler->scale_keep(in->frame);               // VideoCtx::send_frame -> DynamicScaler::scale (encode.rs:287-295)
    }
    ticks.push_back(std::move(mt));
}

MonitorState::Layout MonitorState::layout() const {
    Layout l{};
    l.width = scaler->out_w(); l.height = scaler->out_h();
    size_t total = 0;                                   // DFrame's own layout for yuv420p (mx_video.cpp alloc_planes): what every kept frame has
    for (int p = 0; p < 3; ++p) {
        const uint32_t rb = p ? l.width >> 1 : l.width, rows = p ? l.height >> 1 : l.height;
        l.stride[p] = (rb + 63u) & ~63u;
        l.plane_offset[p] = total;
        total += ((size_t)l.stride[p] * rows + 255) & ~(size_t)255;
    }
    l.frame_bytes = total;
    return l;
}

// ---- video scope taps (mixlab_gpu.h mx_graph_set_video_scopes) ----
void VideoScopeTaps::set(const mx_port_ref* ports, size_t n, const mx_video_scope_params* params) {
    hip_check(hipSetDevice(host_.device()), "hipSetDevice");
    if (n && (!ports || !params)) throw Error(MX_ERR_INVALID, "ports / params is NULL");
    if (n > 0xffffffu) throw Error(MX_ERR_INVALID, "more than 2^24 video scope taps");
    if (n) {
        const uint32_t C = params->wave_cols;
        if (C != 0 && C != 64 && C != 128 && C != 256) throw Error(MX_ERR_INVALID, "mx_video_scope_params: wave_cols must be 0, 64, 128 or 256");
        if (params->hop == 0) throw Error(MX_ERR_INVALID, "mx_video_scope_params: hop must be >= 1");
    }
    std::vector<uint64_t> keys(n);
    for (size_t i = 0; i < n; ++i) {
        const int line = host_.out_line(ports[i]);
        if (line < 0) throw Error(MX_ERR_INVALID, "video scope: output terminal out of range");
        if (line != MX_VIDEO) throw Error(MX_ERR_TYPE, "video scope: an audio port has no picture (meters and spectrum taps observe audio ports)");
        keys[i] = (uint64_t)ports[i].node << 32 | ports[i].port;
    }
    std::sort(keys.begin(), keys.end());
    if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) throw Error(MX_ERR_INVALID, "video scope: duplicate (node, port)");
    size_t rec_bytes = 0, cap = 0;
    if (n) {
        rec_bytes = scope_record_bytes(params->wave_cols, params->vectorscope);
        const size_t max_ticks = std::max<size_t>(1, host_.cap_frames() / host_.spt());
        cap = (max_ticks + params->hop - 1) / params->hop;
        const unsigned __int128 need = (unsigned __int128)cap * n * rec_bytes;
        if (need > ((unsigned __int128)4 << 30))
            throw Error(MX_ERR_NOMEM, "video scopes: the records of one run (ceil(max_ticks_per_run / hop) x taps x record bytes) exceed 4 GiB: raise hop");
    }
    host_.sync();   // the last run's launches are done with the records
    ports_.assign(ports, ports + n);
    hop_.reset(); n_rec_ = 0; run_seen_ = false; now_ = false;
    rec_.free_();
    rec_bytes_ = rec_bytes; cap_ = cap;
    if (ports_.empty()) { par_ = mx_video_scope_params{0, 0, 1}; return; }
    par_ = *params;
    hop_.reset(par_.hop);
    rec_.alloc(cap * n * rec_bytes);
}

void VideoScopeTaps::begin_run(uint32_t n_calls) {
    if (ports_.empty()) return;
    const size_t n_rec = (size_t)hop_.begin_run(n_calls).count;
    if (n_rec > cap_) throw Error(MX_ERR_INTERNAL, "video scopes: the run records more ticks than the taps were sized for");
    if (n_rec) hip_check(hipMemsetAsync(rec_.p, 0, n_rec * ports_.size() * rec_bytes_, host_.stream()), "hipMemsetAsync(video scope records)");
    n_rec_ = 0; run_seen_ = true;
}

// One tap's record of the tick being run.  Ordering: everything is on the graph's stream -- a graph with video nodes never runs anything on the second
// stream (it excludes that mode), the run's fill of the records went out on the stream before its first launch, a frame's producer
// (a cross-fade, a scaler, a band scaler) launched on the stream or is launched here (ensure_pixels, then the queued scaler jobs), and whoever
// writes the frame's memory again is queued behind this launch.  A symbolic frame is materialised: the consumers downstream then read its
// planes instead of re-evaluating the chain -- the same bytes, every cross-fade step truncates to u8 wherever it runs.
void VideoScopeTaps::launch(uint32_t tap) {
    const hipStream_t s = host_.stream();
    ScopeArgs a{};
    a.wave_cols = par_.wave_cols; a.vectorscope = par_.vectorscope;
    a.tick_in_run = tick_in_run_;
    a.rec = reinterpret_cast<uint32_t*>((uint8_t*)rec_.p + ((size_t)n_rec_ * ports_.size() + tap) * rec_bytes_);
    if (DFrame* d = host_.video_out(ports_[tap]).frame.f) {
        a.present = 1;
        a.pixfmt = (d->fmt == MX_PIXFMT_YUV420P && d->with_alpha) ? (uint32_t)MX_PIXFMT_YUVA420P : d->fmt;
        a.width = d->width; a.height = d->height;
        if (d->fmt == MX_PIXFMT_YUV420P) {
            d->ensure_pixels(s);
            flush_scales(s);   // a scaler output just asked for (or queued earlier in the tick) must be written before it is read
            a.counted = 1;
            a.y = d->data[0]; a.u = d->data[1]; a.v = d->data[2];
            a.y_stride = d->stride[0]; a.u_stride = d->stride[1]; a.v_stride = d->stride[2];
        }
    }
    launch_video_scope(a, s);
}

size_t VideoScopeTaps::read(void* dst, size_t cap_bytes) {
    hip_check(hipSetDevice(host_.device()), "hipSetDevice");
    if (ports_.empty()) throw Error(MX_ERR_INVALID, "no video scope taps are set");
    if (!run_seen_) throw Error(MX_ERR_INVALID, "no run since the video scope taps were set");
    const size_t count = (size_t)n_rec_ * ports_.size(), bytes = count * rec_bytes_;
    if (cap_bytes < bytes) throw Error(MX_ERR_INVALID, "cap_bytes is smaller than recorded ticks x taps x record bytes");
    if (bytes && !dst) throw Error(MX_ERR_INVALID, "dst is NULL");
    if (bytes) {
        host_.join_tail();
        hip_check(hipMemcpyAsync(dst, rec_.p, bytes, hipMemcpyDeviceToHost, host_.stream()), "hipMemcpyAsync(D2H)");
        host_.sync();
    }
    return count;
}

// ---- the multiviewer (mixlab_gpu.h mx_graph_set_multiview) ----
void MultiviewTap::set(const mx_port_ref* ports, size_t n, const mx_multiview_params* params) {
    if (n && (!ports || !params)) throw Error(MX_ERR_INVALID, "ports / params is NULL");
    if (n) {
        if (n != params->n_views) throw Error(MX_ERR_INVALID, "multiview: n must equal params->n_views");
        check_multiview_params(*params, true);
        for (size_t i = 0; i < n; ++i) {
            const int line = host_.out_line(ports[i]);
            if (line < 0) throw Error(MX_ERR_INVALID, "multiview: output terminal out of range");
            if (line != MX_VIDEO) throw Error(MX_ERR_TYPE, "multiview: an audio port has no picture");
        }
    }
    hip_check(hipSetDevice(host_.device()), "hipSetDevice");
    host_.sync();   // the last run's launch is done with the tables and the pool
    ports_.assign(ports, ports + n);
    last_ = -1; now_ = false; run_seen_ = false;
    clear(); tabs_ = MultiviewTabs{};
    status_ = mx_multiview_status{0, 0, 0, 0};
    par_ = mx_multiview_params{};
    if (n) par_ = *params;
    hop_.reset(n ? par_.hop : 1);
}

void MultiviewTap::begin_run(uint32_t n_calls) {
    if (ports_.empty()) return;
    const HopCounter::Run r = hop_.begin_run(n_calls);
    last_ = r.count ? (int64_t)(r.first + (r.count - 1) * hop_.hop) : -1;
    out_ = FrameRef(); status_ = mx_multiview_status{(uint32_t)r.count, 0, 0, 0}; run_seen_ = true;
}

// The canvas of the tick being run.  Ordering as for a scope tap (VideoScopeTaps::launch): everything is on the graph's stream; a symbolic frame is materialised
// first -- the consumers that ran earlier in the tick evaluated the chain themselves, and those of later ticks read the same bytes -- then the queued scaler jobs
// leave, then the ONE launch.  The canvas is a pool frame nothing but the pool holds: its last reader is on the stream already, or is the caller, who let go of it.
void MultiviewTap::render(uint32_t tick_in_run) {
    const hipStream_t s = host_.stream();
    DFrame* in[MX_MULTIVIEW_MAX] = {};
    uint32_t present = 0;
    for (uint32_t i = 0; i < (uint32_t)ports_.size(); ++i) {
        DFrame* d = host_.video_out(ports_[i]).frame.f;
        if (!d) continue;
        present |= 1u << i;
        if (d->fmt != MX_PIXFMT_YUV420P) continue;   // another pixel format: present, not shown
        d->ensure_pixels(s);
        in[i] = d;
    }
    flush_scales(s);   // a scaler output just asked for (or queued earlier in the tick) must be written before it is read
    FrameRef o = pool_.take([](const DFrame&) { return true; },
                            [&] { return DFrame::create_unfilled(par_.canvas_w, par_.canvas_h, MX_PIXFMT_YUV420P, false); });   // the kernel writes every byte
    status_.shown_mask = multiview_into(in, par_, tabs_, o.f, s);
    status_.present_mask = present;
    status_.tick_in_run = tick_in_run;
    out_ = o;
}

FrameRef MultiviewTap::output(mx_multiview_status* status) {
    if (ports_.empty()) throw Error(MX_ERR_INVALID, "no multiview is set");
    if (!run_seen_) throw Error(MX_ERR_INVALID, "no run since the multiview was set");
    hip_check(hipSetDevice(host_.device()), "hipSetDevice");
    if (out_) { host_.join_tail(); host_.sync(); }   // a frame crossing the ABI: its pixels are there, whatever stream the caller reads them on
    if (status) *status = status_;
    return out_;
}

// ---- video sub-graph: one Engine::run_tick pass over the video nodes in run order ----
void Graph::run_video_tick(uint64_t t, uint32_t tick_in_run) {
    scopes_.begin_tick(tick_in_run);
    multiview_.begin_tick();
    auto input = [&](const Node& n, int i) -> const Node::VOut* {   // Disconnected => None (io.rs:56-57)
        const PortRef pr = n.in_src[i];
        return pr.node < 0 ? nullptr : &nodes_[pr.node].vout[pr.port];
    };
    for (uint32_t id : plan_.video_order) {
        Node& n = nodes_[id];
        switch (n.kind) {
        case MX_KIND_SOURCE_VIDEO:
            n.vout[0] = Node::VOut{};   // Output::from_line_type(Video) = None every tick (io.rs:76) -- and the last tick's frame is let go of before a pool is asked for this tick's
            n.vout[0] = n.vsrc->due(t / spt_, stream_);
            break;
        case MX_KIND_VIDEO_MIXER: {
            VideoInput in[4];
            for (int i = 0; i < 4; ++i) {
                const Node::VOut* v = input(n, i);
                if (!v || !v->frame) continue;
                in[i].frame = v->frame.f; in[i].duration_hint = v->dur; in[i].tick_offset = v->off;
            }
            FrameRef o, a, b;
            n.vmixer->run_tick(t, in, o, a, b);
            n.vout[0] = Node::VOut{o, Rational::make(1, (int64_t)tps_), Rational::make(0, 1)};   // video_mixer.rs:241-247
            // A / B are clones of the input VideoFrames, duration and offset included (video_mixer.rs:80-90)
            mx_video_mixer_params p; std::memcpy(&p, n.params.data(), sizeof p);
            n.vout[1] = Node::VOut{}; n.vout[2] = Node::VOut{};
            if (a && p.a >= 0 && p.a < 4) n.vout[1] = Node::VOut{a, in[p.a].duration_hint, in[p.a].tick_offset};
            if (b && p.b >= 0 && p.b < 4) n.vout[2] = Node::VOut{b, in[p.b].duration_hint, in[p.b].tick_offset};
            break;
        }
        case MX_KIND_MONITOR: n.mon->run_tick(Rational::make((int64_t)t, (int64_t)sample_rate_), input(n, 0)); break;
        case MX_KIND_VIDEO_TO_RGBA: {
            mx_video_to_rgba_params p; std::memcpy(&p, n.params.data(), sizeof p);
            n.rgba->run_tick(input(n, 0), p, *this);
            break;
        }
        default: break;
        }
        scopes_.node_ran(id);
    }
    scopes_.end_tick();
    multiview_.end_tick(tick_in_run);
}

const Node& Graph::node_of_kind(uint32_t node, uint32_t kind, const char* what) const {
    if (node >= nodes_.size() || nodes_[node].kind != kind) throw Error(MX_ERR_INVALID, std::string("node is not a ") + what);
    return nodes_[node];
}

void Graph::set_video_source(uint32_t node, DFrame* frame, Rational dur, Rational off, bool repeat) {
    VideoSourceState& v = *node_of_kind(node, MX_KIND_SOURCE_VIDEO, "SOURCE_VIDEO").vsrc;
    v.frame = frame ? FrameRef(frame, true) : FrameRef();
    v.dur = dur; v.off = off; v.repeat = repeat; v.pending = frame != nullptr;
}

void Graph::set_video_source_band(uint32_t node, uint32_t in_w, uint32_t in_full_h, uint32_t src_row0, uint32_t slice_rows,
                                  uint32_t full_w, uint32_t full_h, uint32_t row0, uint32_t band_rows) {
    VideoSourceState& v = *node_of_kind(node, MX_KIND_SOURCE_VIDEO, "SOURCE_VIDEO").vsrc;
    if (band_rows && v.transform.grade_on()) throw Error(MX_ERR_INVALID, "video source band: the source is graded (mx_graph_set_video_source_grade); grading a band-scaled layer is not supported");
    if (band_rows && v.transform.key_on()) throw Error(MX_ERR_INVALID, "video source band: the source is keyed (mx_graph_set_video_source_key), and a band-scaled layer cannot carry coverage");
    if (band_rows && v.transform.matte_on()) throw Error(MX_ERR_INVALID, "video source band: the source is matted (mx_graph_set_video_source_matte), and a band-scaled layer cannot carry coverage");
    if (band_rows && v.transform.place_on()) throw Error(MX_ERR_INVALID, "video source band: the source is placed (mx_graph_set_video_source_place), and a band-scaled layer cannot carry coverage");
    sync();                                     // a previous band scaler's row buffer may be in use
    v.band.reset(); v.band_pool.clear();
    if (band_rows) v.band = std::make_shared<BandScaler>(in_w, in_full_h, src_row0, slice_rows, full_w, full_h, row0, band_rows);
}

void Graph::set_video_source_key(uint32_t node, const mx_video_key_params* params) {
    if (node >= nodes_.size()) throw Error(MX_ERR_INVALID, "node out of range");
    if (nodes_[node].kind != MX_KIND_SOURCE_VIDEO) throw Error(MX_ERR_TYPE, "video source key: node is not a SOURCE_VIDEO");
    VideoSourceState& v = *nodes_[node].vsrc;
    if (params) {
        check_key_params(*params);
        if (v.band) throw Error(MX_ERR_INVALID, "video source key: the source delivers a row band of a scaled layer (mx_graph_set_video_source_band), which cannot carry coverage");
    }
    v.transform.set_key(params);
}

void Graph::set_video_source_grade(uint32_t node, const mx_video_grade_params* params, std::shared_ptr<const LutTables> lut) {
    if (node >= nodes_.size()) throw Error(MX_ERR_INVALID, "node out of range");
    if (nodes_[node].kind != MX_KIND_SOURCE_VIDEO) throw Error(MX_ERR_TYPE, "video source grade: node is not a SOURCE_VIDEO");
    VideoSourceState& v = *nodes_[node].vsrc;
    if (params) {
        check_grade_params(*params, lut != nullptr);
        if (v.band) throw Error(MX_ERR_INVALID, "video source grade: the source delivers a row band of a scaled layer (mx_graph_set_video_source_band); grading a band-scaled layer is not supported");
    }
    v.transform.set_grade(params, std::move(lut));
}

void Graph::set_video_source_matte(uint32_t node, const mx_video_matte_params* params) {
    if (node >= nodes_.size()) throw Error(MX_ERR_INVALID, "node out of range");
    if (nodes_[node].kind != MX_KIND_SOURCE_VIDEO) throw Error(MX_ERR_TYPE, "video source matte: node is not a SOURCE_VIDEO");
    VideoSourceState& v = *nodes_[node].vsrc;
    if (params) {
        check_matte_params(*params);
        if (v.band) throw Error(MX_ERR_INVALID, "video source matte: the source delivers a row band of a scaled layer (mx_graph_set_video_source_band), which cannot carry coverage");
    }
    v.transform.set_matte(params);
}

void Graph::set_video_source_place(uint32_t node, const mx_video_place_params* params) {
    if (node >= nodes_.size()) throw Error(MX_ERR_INVALID, "node out of range");
    if (nodes_[node].kind != MX_KIND_SOURCE_VIDEO) throw Error(MX_ERR_TYPE, "video source place: node is not a SOURCE_VIDEO");
    VideoSourceState& v = *nodes_[node].vsrc;
    if (params) {
        check_place_params(*params);
        if (v.band) throw Error(MX_ERR_INVALID, "video source place: the source delivers a row band of a scaled layer (mx_graph_set_video_source_band), which cannot carry coverage");
    }
    v.transform.set_place(params);
}

void Graph::queue_video_source(uint32_t node, uint64_t tick, DFrame* frame, Rational dur, Rational off) {
    (void)node_of_kind(node, MX_KIND_SOURCE_VIDEO, "SOURCE_VIDEO");
    if (!frame) throw Error(MX_ERR_INVALID, "frame is NULL");
    check_video_queue(node, tick);
    nodes_[node].vsrc->sched.push_back(VideoSourceState::Sched{tick, FrameRef(frame, true), dur, off});
}

void Graph::check_video_queue(uint32_t node, uint64_t first_tick) const {
    const VideoSourceState& v = *node_of_kind(node, MX_KIND_SOURCE_VIDEO, "SOURCE_VIDEO").vsrc;
    if (!v.sched.empty() && v.sched.back().tick >= first_tick) throw Error(MX_ERR_INVALID, "video source frames must be queued in tick order, one per tick");
}

void Graph::check_source_write(uint32_t node, size_t frames) const {
    if (node >= nodes_.size()) throw Error(MX_ERR_INVALID, "node out of range");
    const Node& n = nodes_[node];
    if (n.kind != MX_KIND_SOURCE_MONO && n.kind != MX_KIND_SOURCE_STEREO) throw Error(MX_ERR_INVALID, "node is not a SOURCE_*");
    if (n.bound) throw Error(MX_ERR_INVALID, "source is bound to a caller device buffer");
    if (frames > cap_frames_) throw Error(MX_ERR_INVALID, "more ticks than max_ticks_per_run");
}

void Graph::monitor_consume(uint32_t node, uint32_t n_ticks) {
    MonitorState& m = *node_of_kind(node, MX_KIND_MONITOR, "MONITOR").mon;
    m.queued -= std::min(m.queued, n_ticks);
}

const Node::MonTick& Graph::monitor_tick(uint32_t node, uint32_t tick_in_run) {
    const MonitorState& m = *node_of_kind(node, MX_KIND_MONITOR, "MONITOR").mon;
    if (tick_in_run >= m.ticks.size()) throw Error(MX_ERR_INVALID, "tick_in_run beyond the last run");
    flush_scales(stream_);
    sync();          // the caller reads the frame on streams of its own
    return m.ticks[tick_in_run];
}

Graph::MonitorLayout Graph::monitor_layout(uint32_t node) { return node_of_kind(node, MX_KIND_MONITOR, "MONITOR").mon->layout(); }

void Graph::read_monitor_video(uint32_t node, uint32_t first_tick, uint32_t n_ticks, uint8_t* frames, uint8_t* present) {
    MonitorState& m = *node_of_kind(node, MX_KIND_MONITOR, "MONITOR").mon;
    const MonitorLayout l = m.layout();
    if ((size_t)first_tick + n_ticks > m.ticks.size()) throw Error(MX_ERR_INVALID, "ticks beyond the last run");
    if (n_ticks && (!frames || !present)) throw Error(MX_ERR_INVALID, "NULL argument");
    if (!n_ticks) return;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    const size_t need = (size_t)n_ticks * l.frame_bytes;
    if (m.pack.bytes < need) { sync(); m.pack.alloc(need); }
    uint32_t any = 0;
    for (uint32_t k0 = 0; k0 < n_ticks; k0 += 224) {
        GatherArgs a{};
        a.n = std::min<uint32_t>(224u, n_ticks - k0);
        a.dst = reinterpret_cast<uint4*>((uint8_t*)m.pack.p + (size_t)k0 * l.frame_bytes);
        a.q_per_frame = (uint32_t)(l.frame_bytes / 16);
        for (uint32_t k = 0; k < a.n; ++k) {
            const Node::MonTick& mt = m.ticks[first_tick + k0 + k];
            present[k0 + k] = mt.present ? 1 : 0;
            a.src[k] = nullptr;
            if (!mt.present) continue;
            const DFrame* f = mt.frame.f;
            if (f->mem.bytes != l.frame_bytes || f->plane_offset(1) != l.plane_offset[1] || f->plane_offset(2) != l.plane_offset[2])
                throw Error(MX_ERR_INTERNAL, "a kept monitor frame does not have the monitor layout");
            a.src[k] = reinterpret_cast<const uint4*>(f->mem.p);
            ++any;
        }
        launch_gather_frames(a, stream_);
    }
    if (any) hip_check(hipMemcpyAsync(frames, m.pack.p, need, hipMemcpyDeviceToHost, stream_), "hipMemcpyAsync(D2H monitor frames)");
    sync();
}

void Graph::read_monitor_audio_i16(uint32_t node, int16_t* host, uint32_t n_ticks) {
    const PortRef pr = node_of_kind(node, MX_KIND_MONITOR, "MONITOR").in_src[1];
    if (n_ticks > last_calls_) throw Error(MX_ERR_INVALID, "more ticks than the last run had");
    if (n_ticks && !host) throw Error(MX_ERR_INVALID, "audio is NULL");
    const size_t per_tick = 2 * last_frames_per_call_;
    if (pr.node < 0) { std::memset(host, 0, (size_t)n_ticks * per_tick * sizeof(int16_t)); return; }   // InputRef::Disconnected: the zero buffer
    read_output_i16((uint32_t)pr.node, (uint32_t)pr.port, host, (size_t)n_ticks * last_frames_per_call_);
}

void Graph::set_video_source_ring(uint32_t node, DFrame* const* frames, size_t n, Rational dur, Rational off) {
    VideoSourceState& v = *node_of_kind(node, MX_KIND_SOURCE_VIDEO, "SOURCE_VIDEO").vsrc;
    v.ring.clear(); v.ring_pos = 0;
    for (size_t i = 0; i < n; ++i) v.ring.push_back(FrameRef(frames[i], true));
    v.dur = dur; v.off = off;
    if (n) { v.frame = FrameRef(); v.pending = false; v.repeat = false; }
}

FrameRef Graph::video_output(uint32_t node, uint32_t port) {
    if (node >= nodes_.size() || port >= nodes_[node].vout.size() || nodes_[node].out_type[port] != MX_VIDEO)
        throw Error(MX_ERR_INVALID, "not a video output terminal");
    FrameRef r = nodes_[node].vout[port].frame;
    if (r) {   // a frame crossing the ABI must have pixels -- and they must be there: the caller reads them on whatever stream it likes
        r->ensure_pixels(stream_);
        flush_scales(stream_);
        sync();
    }
    return r;
}

void Graph::rgba_output(uint32_t node, void** dev, int32_t* stride, uint32_t* w, uint32_t* h) {
    const RgbaSinkState& r = *node_of_kind(node, MX_KIND_VIDEO_TO_RGBA, "VIDEO_TO_RGBA").rgba;
    if (dev) *dev = r.w ? r.buf[r.cur].p : nullptr;
    if (stride) *stride = r.stride;
    if (w) *w = r.w;
    if (h) *h = r.h;
}

}  // namespace mx

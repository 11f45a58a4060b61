// mx_abi_deck.cpp -- extern "C" entry points of the deck (include/mixlab_gpu.h, "the deck").
// Same fencing convention as mx_abi.cpp: catch everything, stash the message, return a status.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mx_deck.hpp"
#include "mx_deck_waveform.hpp"
#include "mx_engine.hpp"
#include "mx_video.hpp"
#include "mx_abi_common.hpp"

using mx::Deck;
using mx::Error;

struct mx_deck { Deck d; mx_deck(uint64_t n_frames, int device) : d(n_frames, device) {} };


extern "C" {

int mx_deck_create(uint64_t n_frames, int device, mx_deck** out) {
    return guard([&] { REQUIRE(out, "out is NULL"); *out = nullptr; *out = new mx_deck(n_frames, device); });
}
void mx_deck_destroy(mx_deck* d) { (void)guard([&] { delete d; }); }

int mx_deck_load_i16(mx_deck* d, uint64_t first_frame, const int16_t* interleaved, uint64_t n_frames) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.load_i16(first_frame, interleaved, n_frames); });
}
int mx_deck_set(mx_deck* d, const mx_deck_params* params) {
    return guard([&] { REQUIRE(d && params, "NULL argument"); d->d.schedule(0, params, nullptr); });
}
int mx_deck_seek(mx_deck* d, int64_t pos_q32) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.schedule(0, nullptr, &pos_q32); });
}
int mx_deck_schedule(mx_deck* d, uint32_t tick_in_feed, const mx_deck_params* params, const int64_t* seek_pos_q32) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.schedule(tick_in_feed, params, seek_pos_q32); });
}
int mx_deck_check(const mx_deck_params* params, uint64_t n_frames) {
    return guard([&] { REQUIRE(params, "params is NULL"); mx::deck_check(*params, n_frames); });
}
int mx_deck_plan(const mx_deck_head* in, const mx_deck_params* params, const int64_t* seek_pos_q32, uint32_t spt, uint64_t n_frames, mx_deck_tick* tick, mx_deck_head* out) {
    return guard([&] { REQUIRE(in && tick && out, "NULL argument"); mx::deck_plan(*in, params, seek_pos_q32, spt, n_frames, *tick, *out); });
}
int mx_deck_feed(mx_deck* const* decks, const uint32_t* nodes, size_t n, mx_graph* g, uint32_t n_ticks) {
    return guard([&] {
        REQUIRE(g, "graph is NULL");
        REQUIRE(!n || (decks && nodes), "decks / nodes is NULL");
        std::vector<Deck*> ds(n);
        for (size_t i = 0; i < n; ++i) ds[i] = decks[i] ? &decks[i]->d : nullptr;
        Deck::feed(ds.data(), nodes, n, *g->g, n_ticks);
    });
}
int mx_deck_read_ticks(const mx_deck* d, uint32_t first, uint32_t n, mx_deck_tick* dst) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.read_ticks(first, n, dst); });
}
int mx_deck_state(const mx_deck* d, mx_deck_head* out) {
    return guard([&] { REQUIRE(d && out, "NULL argument"); *out = d->d.head(); });
}
int mx_deck_step(uint32_t track_rate, uint32_t graph_rate, double speed, int64_t* step_q32) {
    return guard([&] { REQUIRE(step_q32, "step_q32 is NULL"); *step_q32 = mx::deck_step(track_rate, graph_rate, speed); });
}
int mx_deck_tables(uint32_t bank, float* out) {
    return guard([&] {
        REQUIRE(out, "out is NULL"); REQUIRE(bank < MX_DECK_BANKS, "bank outside 0 .. 3");
        std::memcpy(out, mx::deck_tables_host() + (size_t)bank * mx::DECK_BANK_FLOATS, (size_t)mx::DECK_BANK_FLOATS * sizeof(float));
    });
}
int mx_deck_debug_last_feed(uint32_t out[6]) {
    return guard([&] { REQUIRE(out, "out is NULL"); Deck::debug_last_feed(out); });
}
int mx_deck_set_keylock(mx_deck* d, const mx_deck_keylock* k) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.set_keylock(k); });
}
int mx_deck_keylock_check(const mx_deck_keylock* k) {
    return guard([&] { REQUIRE(k, "settings are NULL"); mx::deck_keylock_check(*k); });
}
int mx_deck_keylock_search(const int16_t* interleaved, uint64_t n_frames, int64_t C, int64_t A, uint32_t overlap, uint32_t radius, int32_t* delta, uint32_t* dist) {
    return guard([&] { REQUIRE(delta && dist, "NULL argument"); mx::deck_keylock_search(interleaved, n_frames, C, A, overlap, radius, *delta, *dist); });
}
int mx_deck_grain_count(const mx_deck* d, uint32_t* n) {
    return guard([&] { REQUIRE(d && n, "NULL argument"); *n = d->d.grain_count(); });
}
int mx_deck_read_grains(mx_deck* d, uint32_t first, uint32_t n, mx_deck_grain* dst) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.read_grains(first, n, dst); });
}
int mx_deck_debug_last_keylock(uint32_t out[4]) {
    return guard([&] { REQUIRE(out, "out is NULL"); Deck::debug_last_keylock(out); });
}
int mx_deck_set_echo(mx_deck* d, const mx_deck_echo* e) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.echo.schedule(0, e); });
}
int mx_deck_schedule_echo(mx_deck* d, uint32_t tick_in_feed, const mx_deck_echo* e) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.echo.schedule(tick_in_feed, e); });
}
int mx_deck_echo_check(const mx_deck_echo* e) {
    return guard([&] { REQUIRE(e, "settings are NULL"); mx::deck_echo_check(*e); });
}
int mx_deck_echo_state(const mx_deck* d, uint64_t* t, uint32_t* on, mx_deck_echo* setting) {
    return guard([&] {
        REQUIRE(d && t && on && setting, "NULL argument");
        const mx::DeckEcho::State& s = d->d.echo.state();
        *t = s.t; *on = s.on ? 1u : 0u; *setting = s.set;
    });
}
int mx_deck_echo_plan(uint32_t spt, const uint32_t* delay, uint32_t n_ticks, uint64_t* blocks, uint32_t cap, uint32_t* n_blocks) {
    return guard([&] {
        REQUIRE(n_blocks && (delay || !n_ticks) && (blocks || !cap), "NULL argument");
        REQUIRE(spt >= 1 && spt <= MX_DECK_MAX_SPT, "frames per tick outside 1 .. MX_DECK_MAX_SPT");
        for (uint32_t k = 0; k < n_ticks; ++k)
            REQUIRE(!delay[k] || (delay[k] >= MX_DECK_ECHO_MIN_DELAY && delay[k] <= MX_DECK_ECHO_MAX_DELAY), "a delay that is neither 0 nor in MX_DECK_ECHO_MIN_DELAY .. MX_DECK_ECHO_MAX_DELAY");
        std::vector<mx::EchoBlock> cut;
        mx::deck_echo_cut(spt, delay, n_ticks, cut);
        REQUIRE(cut.size() <= 0xffffffffu, "more than 2^32 blocks");
        *n_blocks = (uint32_t)cut.size();
        for (size_t k = 0; k < cut.size() && k < cap; ++k) { blocks[2 * k] = cut[k].first; blocks[2 * k + 1] = cut[k].frames; }
    });
}
int mx_deck_debug_last_echo(uint32_t out[4]) {
    return guard([&] { REQUIRE(out, "out is NULL"); mx::deck_debug_last_echo(out); });
}
int mx_deck_set_filter(mx_deck* d, const mx_deck_filter* f) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.filter.schedule(0, f); });
}
int mx_deck_schedule_filter(mx_deck* d, uint32_t tick_in_feed, const mx_deck_filter* f) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.filter.schedule(tick_in_feed, f); });
}
int mx_deck_filter_check(const mx_deck_filter* f) {
    return guard([&] { REQUIRE(f, "settings are NULL"); mx::deck_filter_check(*f); });
}
int mx_deck_filter_state(const mx_deck* d, uint32_t* on, mx_deck_filter* setting) {
    return guard([&] {
        REQUIRE(d && on && setting, "NULL argument");
        const mx::DeckFilter::State& s = d->d.filter.state();
        *on = s.on ? 1u : 0u; *setting = s.set;
    });
}
int mx_deck_read_filter_state(mx_deck* d, double s[4]) {
    return guard([&] { REQUIRE(d && s, "NULL argument"); d->d.filter.read_state(s); });
}
int mx_deck_filter_design(uint32_t kind, double cutoff_hz, double q, double rate, double wet, mx_deck_filter* out) {
    return guard([&] { REQUIRE(out, "out is NULL"); mx::deck_filter_design(kind, cutoff_hz, q, rate, wet, *out); });
}
int mx_deck_filter_knob(double knob, double rate, double q, mx_deck_filter* out, uint32_t* on) {
    return guard([&] { REQUIRE(out && on, "NULL argument"); mx::deck_filter_knob(knob, rate, q, *out, *on); });
}
int mx_deck_filter_host(float* frames, uint32_t spt, uint32_t n_ticks, const mx_deck_filter* const* settings, mx_deck_filter_carry* carry) {
    return guard([&] {
        REQUIRE(carry && (!n_ticks || (frames && settings)), "NULL argument");
        mx::deck_filter_host(frames, spt, n_ticks, settings, *carry);
    });
}
int mx_deck_set_reverb(mx_deck* d, const mx_deck_reverb* r) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.reverb.schedule(0, r); });
}
int mx_deck_schedule_reverb(mx_deck* d, uint32_t tick_in_feed, const mx_deck_reverb* r) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.reverb.schedule(tick_in_feed, r); });
}
int mx_deck_reverb_check(const mx_deck_reverb* r) {
    return guard([&] { REQUIRE(r, "settings are NULL"); mx::deck_reverb_check(*r); });
}
int mx_deck_reverb_state(const mx_deck* d, uint64_t* t, uint32_t* on, mx_deck_reverb* setting) {
    return guard([&] {
        REQUIRE(d && t && on && setting, "NULL argument");
        const mx::DeckReverb::State& s = d->d.reverb.state();
        *t = s.t; *on = s.on ? 1u : 0u; *setting = s.set;
    });
}
int mx_deck_read_reverb_lines(mx_deck* d, float* dst) {
    return guard([&] { REQUIRE(d && dst, "NULL argument"); d->d.reverb.read_lines(dst); });
}
int mx_deck_reverb_plan(uint32_t spt, const mx_deck_reverb* const* settings, uint32_t n_ticks, uint64_t* blocks, uint32_t cap, uint32_t* n_blocks) {
    return guard([&] {
        REQUIRE(n_blocks && (!n_ticks || settings) && (!cap || blocks), "NULL argument");
        REQUIRE(spt >= 1 && spt <= MX_DECK_MAX_SPT, "frames per tick outside 1 .. MX_DECK_MAX_SPT");
        std::vector<uint32_t> reach(n_ticks, 0u);
        for (uint32_t k = 0; k < n_ticks; ++k) if (settings[k]) { mx::deck_reverb_check(*settings[k]); reach[k] = mx::reverb_reach(*settings[k]); }
        std::vector<mx::ReverbBlock> cut;
        mx::deck_reverb_cut(spt, reach.data(), n_ticks, cut);
        REQUIRE(cut.size() <= 0xffffffffu, "more than 2^32 blocks");
        for (size_t j = 0; j < cut.size() && j < cap; ++j) { blocks[2 * j] = cut[j].first; blocks[2 * j + 1] = cut[j].frames; }
        *n_blocks = (uint32_t)cut.size();
    });
}
int mx_deck_reverb_host(float* frames, uint32_t spt, uint32_t n_ticks, const mx_deck_reverb* const* settings, float* lines, mx_deck_reverb_carry* carry) {
    return guard([&] {
        REQUIRE(carry && lines && (!n_ticks || (frames && settings)), "NULL argument");
        mx::deck_reverb_host(frames, spt, n_ticks, settings, lines, *carry);
    });
}
int mx_deck_reverb_design(double rate, double size, double t60_seconds, double damp, double diffusion, double send, double dry, double wet, mx_deck_reverb* out) {
    return guard([&] { REQUIRE(out, "out is NULL"); mx::deck_reverb_design(rate, size, t60_seconds, damp, diffusion, send, dry, wet, *out); });
}
int mx_deck_debug_last_reverb(uint32_t out[4]) {
    return guard([&] { REQUIRE(out, "out is NULL"); mx::deck_debug_last_reverb(out); });
}
int mx_deck_debug_last_filter(uint32_t out[4]) {
    return guard([&] { REQUIRE(out, "out is NULL"); const mx::DeckLastFilter last = mx::deck_last_filter(); for (int k = 0; k < 4; ++k) out[k] = last.out[k]; });
}
int mx_deck_analysis_check(const mx_deck_analysis* a) {
    return guard([&] { REQUIRE(a, "settings are NULL"); mx::deck_analysis_check(*a); });
}
int mx_deck_analysis_bands(double rate, double f_lo, double f_hi, uint32_t taps, mx_deck_analysis* a) {
    return guard([&] { REQUIRE(a, "settings are NULL"); mx::deck_analysis_bands(rate, f_lo, f_hi, taps, *a); });
}
int mx_deck_analyse(mx_deck* d, const mx_deck_analysis* a) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.columns.analyse(a); });
}
int mx_deck_column_count(uint64_t n_frames, uint32_t column, uint64_t* n) {
    return guard([&] { REQUIRE(n, "n is NULL"); *n = mx::deck_column_count(n_frames, column); });
}
int mx_deck_read_columns(mx_deck* d, uint64_t first, uint64_t n, mx_deck_column* dst) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.columns.read_columns(first, n, dst); });
}
int mx_deck_read_autocorr(mx_deck* d, uint64_t* R, uint32_t cap) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.columns.read_autocorr(R, cap); });
}
int mx_deck_columns_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_analysis* a, uint64_t first, uint64_t n, mx_deck_column* cols, uint64_t* R_or_null) {
    return guard([&] { REQUIRE(a, "settings are NULL"); mx::deck_columns_host(interleaved, n_frames, *a, first, n, cols, R_or_null); });
}
int mx_deck_beatgrid(const mx_deck_column* cols, uint64_t n_cols, const uint64_t* R, uint32_t max_lag, uint32_t column, double rate, double bpm_lo, double bpm_hi,
                     mx_deck_grid* out) {
    return guard([&] { REQUIRE(out, "out is NULL"); mx::deck_beatgrid(cols, n_cols, R, max_lag, column, rate, bpm_lo, bpm_hi, *out); });
}
int mx_deck_debug_last_analysis(uint32_t out[4]) {
    return guard([&] { REQUIRE(out, "out is NULL"); mx::DeckColumns::debug_last(out); });
}
int mx_deck_tonality_check(const mx_deck_tonality* t) {
    return guard([&] { REQUIRE(t, "settings are NULL"); mx::deck_tonality_check(*t); });
}
int mx_deck_tonality_count(uint64_t n_frames, const mx_deck_tonality* t, uint64_t* n_seg) {
    return guard([&] { REQUIRE(t && n_seg, "NULL argument"); *n_seg = mx::deck_tonality_count(n_frames, *t); });
}
int mx_deck_analyse_tonality(mx_deck* d, const mx_deck_tonality* t) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.tonality.analyse(t); });
}
int mx_deck_read_tonality(mx_deck* d, uint64_t first, uint64_t n, void* dst, size_t cap_bytes) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.tonality.read(first, n, dst, cap_bytes); });
}
int mx_deck_tonality_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_tonality* t, uint64_t first, uint64_t n, void* dst) {
    return guard([&] { REQUIRE(t, "settings are NULL"); mx::deck_tonality_host(interleaved, n_frames, *t, first, n, dst); });
}
int mx_deck_debug_last_tonality(uint32_t out[4]) {
    return guard([&] { REQUIRE(out, "out is NULL"); mx::DeckTonality::debug_last(out); });
}
int mx_deck_loudness_check(const mx_deck_loudness* l) {
    return guard([&] { REQUIRE(l, "settings are NULL"); mx::deck_loudness_check(*l); });
}
int mx_deck_loudness_count(uint64_t n_frames, uint32_t block_frames, uint64_t* n_blocks) {
    return guard([&] { REQUIRE(n_blocks, "n_blocks is NULL"); *n_blocks = mx::deck_loudness_count(n_frames, block_frames); });
}
int mx_deck_analyse_loudness(mx_deck* d, const mx_deck_loudness* l) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.loudness.analyse(l); });
}
int mx_deck_read_loudness(mx_deck* d, uint64_t first, uint64_t n, mx_loudness_tick* dst) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.loudness.read(first, n, dst); });
}
int mx_deck_loudness_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_loudness* l, mx_loudness_tick* dst, uint64_t cap) {
    return guard([&] { REQUIRE(l, "settings are NULL"); mx::deck_loudness_host(interleaved, n_frames, *l, dst, cap); });
}
int mx_deck_debug_last_loudness(uint32_t out[4]) {
    return guard([&] { REQUIRE(out, "out is NULL"); mx::DeckLoudness::debug_last(out); });
}
int mx_deck_loudness_gain(const mx_loudness_tick* recs, uint64_t n, uint32_t momentary_blocks, uint32_t hop_blocks, double target_lufs, double ceiling_dbtp,
                          double* lufs, double* peak_dbtp, double* gain_db) {
    return guard([&] {
        REQUIRE(recs && lufs && peak_dbtp && gain_db, "NULL argument");
        REQUIRE(n > 0 && hop_blocks > 0, "no records, or hop_blocks is 0");
        REQUIRE(momentary_blocks >= 1 && momentary_blocks <= 1024, "momentary_blocks outside 1 .. 1024");
        REQUIRE(std::isfinite(target_lufs) && std::isfinite(ceiling_dbtp), "target_lufs or ceiling_dbtp is not finite");
        std::vector<double> sq; std::vector<uint32_t> fr;
        for (uint64_t i = std::min<uint64_t>(momentary_blocks - 1, n - 1); i < n; i += hop_blocks) {
            const uint64_t f = (uint64_t)momentary_blocks * recs[i].frames;
            REQUIRE(f > 0 && f <= 0xffffffffu, "a record of 0 frames, or a measurement block beyond 2^32 frames");
            sq.push_back(recs[i].momentary_sq); fr.push_back((uint32_t)f);
        }
        double l = 0.0;
        if (mx_loudness_gate(sq.data(), fr.data(), sq.size(), &l, nullptr) != MX_OK) throw Error(MX_ERR_INVALID, mx_last_error());
        float peak = 0.0f;
        for (uint64_t i = 0; i < n; ++i) peak = std::max(peak, std::max(recs[i].true_peak[0], recs[i].true_peak[1]));
        const double p = peak > 0.0f ? 20.0 * std::log10((double)peak) : -HUGE_VAL;
        *lufs = l; *peak_dbtp = p;
        *gain_db = l == -HUGE_VAL ? 0.0 : std::min(target_lufs - l, ceiling_dbtp - p);
    });
}
int mx_tonality_camelot(int key, uint32_t* number, uint32_t* minor) {
    return guard([&] {
        REQUIRE(number && minor, "NULL argument"); REQUIRE(key >= 0 && key <= 23, "key outside 0 .. 23");
        const int m = key >= 12, t = key - 12 * m;
        *number = (uint32_t)((7 * t + (m ? 4 : 7)) % 12) + 1u; *minor = (uint32_t)m;
    });
}
int mx_deck_finegrid_check(const mx_deck_finegrid* s, uint64_t n_frames) {
    return guard([&] { REQUIRE(s, "settings are NULL"); mx::deck_finegrid_check(*s, n_frames, true); });
}
int mx_deck_finegrid_count(uint64_t n_frames, uint32_t hop, uint64_t* n_hops) {
    return guard([&] { REQUIRE(n_hops, "n_hops is NULL"); *n_hops = mx::deck_finegrid_count(n_frames, hop); });
}
int mx_deck_finegrid_span(uint64_t centre_q16, uint64_t halfwidth_q16, uint32_t beat_limit, uint64_t n_hops, uint32_t hop, mx_deck_finegrid* s, uint32_t* clipped) {
    return guard([&] { REQUIRE(s, "settings are NULL"); mx::deck_finegrid_span(centre_q16, halfwidth_q16, beat_limit, n_hops, hop, *s, clipped); });
}
int mx_deck_finegrid_period(double period_columns, uint32_t column, uint32_t hop, uint64_t* period_q16) {
    return guard([&] { REQUIRE(period_q16, "period_q16 is NULL"); *period_q16 = mx::deck_finegrid_period(period_columns, column, hop); });
}
int mx_deck_analyse_finegrid(mx_deck* d, const mx_deck_finegrid* s) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.finegrid.analyse(s); });
}
int mx_deck_read_finegrid(mx_deck* d, uint64_t first, uint64_t n, mx_deck_comb* dst) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.finegrid.read(first, n, dst); });
}
int mx_deck_read_fine_onsets(mx_deck* d, uint64_t first, uint64_t n, uint32_t* w) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.finegrid.read_onsets(first, n, w); });
}
int mx_deck_finegrid_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_finegrid* s, mx_deck_comb* recs, uint32_t* w_or_null) {
    return guard([&] { REQUIRE(s, "settings are NULL"); mx::deck_finegrid_host(interleaved, n_frames, *s, recs, w_or_null); });
}
int mx_deck_finegrid_pick(const mx_deck_comb* recs, const mx_deck_finegrid* s, double rate, mx_deck_fine_pick* out) {
    return guard([&] { REQUIRE(s && out, "NULL argument"); mx::deck_finegrid_pick(recs, *s, rate, *out); });
}
int mx_deck_sync(const mx_deck_beats* leader, int64_t leader_pos_q32, int64_t leader_step_q32, const mx_deck_beats* follower, int64_t follower_pos_q32,
                 mx_deck_sync_result* out) {
    return guard([&] { REQUIRE(leader && follower && out, "NULL argument"); mx::deck_sync(*leader, leader_pos_q32, leader_step_q32, *follower, follower_pos_q32, *out); });
}
int mx_deck_echo_delay(const mx_deck_beats* grid, int64_t step_q32, uint32_t num, uint32_t den, uint32_t* delay) {
    return guard([&] { REQUIRE(grid && delay, "NULL argument"); *delay = mx::deck_echo_delay(*grid, step_q32, num, den); });
}
int mx_deck_debug_last_finegrid(uint32_t out[4]) {
    return guard([&] { REQUIRE(out, "out is NULL"); mx::DeckFineGrid::debug_last(out); });
}
int mx_deck_bars_check(const mx_deck_bars* s, uint64_t n_frames) {
    return guard([&] { REQUIRE(s, "settings are NULL"); (void)mx::deck_bars_check(*s, n_frames, true); });
}
int mx_deck_bars_count(const mx_deck_bars* s, uint64_t n_frames, uint32_t* n_beats, int64_t* n0) {
    return guard([&] {
        REQUIRE(s, "settings are NULL");
        const mx::BarsBeats b = mx::deck_bars_check(*s, n_frames, true);
        if (n_beats) *n_beats = b.n_beats;
        if (n0) *n0 = b.n0;
    });
}
int mx_deck_bars_tables(const mx_deck_analysis* a, mx_deck_bars* s) {
    return guard([&] { REQUIRE(a && s, "NULL argument"); mx::deck_bars_tables(*a, *s); });
}
int mx_deck_analyse_bars(mx_deck* d, const mx_deck_bars* s) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.bars.analyse(s); });
}
int mx_deck_read_bars(mx_deck* d, uint64_t first, uint64_t n, mx_deck_beat* dst) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.bars.read(first, n, dst); });
}
int mx_deck_read_bar_folds(mx_deck* d, uint64_t* H, uint32_t cap) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.bars.read_folds(H, cap); });
}
int mx_deck_bars_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_bars* s, mx_deck_beat* recs, uint64_t* H_or_null) {
    return guard([&] { REQUIRE(s, "settings are NULL"); mx::deck_bars_host(interleaved, n_frames, *s, recs, H_or_null); });
}
int mx_deck_bars_pick(const uint64_t* H, const mx_deck_bars* s, mx_deck_bar_pick* out) {
    return guard([&] { REQUIRE(s && out, "NULL argument"); mx::deck_bars_pick(H, *s, *out); });
}
int mx_deck_grid_next(const mx_deck_beats* grid, int64_t pos_q32, int64_t* index, int64_t* line_q32) {
    return guard([&] { REQUIRE(grid, "grid is NULL"); mx::deck_grid_next(*grid, pos_q32, index, line_q32); });
}
int mx_deck_debug_last_bars(uint32_t out[4]) {
    return guard([&] { REQUIRE(out, "out is NULL"); mx::DeckBars::debug_last(out); });
}
int mx_deck_tempomap_check(const mx_deck_tempomap* s, uint64_t n_frames) {
    return guard([&] { REQUIRE(s, "settings are NULL"); (void)mx::deck_tempomap_check(*s, n_frames); });
}
int mx_deck_tempomap_count(const mx_deck_tempomap* s, uint64_t n_frames, uint32_t* n_windows) {
    return guard([&] { REQUIRE(s && n_windows, "NULL argument"); *n_windows = mx::deck_tempomap_check(*s, n_frames); });
}
int mx_deck_tempomap_span(uint64_t centre_q16, uint64_t halfwidth_q16, uint32_t window_beats, uint32_t stride_beats, uint64_t n_hops, uint32_t hop, mx_deck_tempomap* s,
                          uint32_t* clipped) {
    return guard([&] { REQUIRE(s, "settings are NULL"); mx::deck_tempomap_span(centre_q16, halfwidth_q16, window_beats, stride_beats, n_hops, hop, *s, clipped); });
}
int mx_deck_tempomap_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_tempomap* s, mx_deck_comb* recs, uint32_t* w_or_null) {
    return guard([&] { REQUIRE(s, "settings are NULL"); mx::deck_tempomap_host(interleaved, n_frames, *s, recs, w_or_null); });
}
int mx_deck_tempomap_path(const mx_deck_comb* recs, uint32_t n_windows, uint32_t n_periods, uint64_t penalty, uint32_t* index) {
    return guard([&] { mx::deck_tempomap_path(recs, n_windows, n_periods, penalty, index); });
}
int mx_deck_tempomap_segments(const mx_deck_comb* recs, const mx_deck_tempomap* s, uint64_t n_frames, const uint32_t* index, mx_deck_tempo_segment* segs) {
    return guard([&] { REQUIRE(s, "settings are NULL"); mx::deck_tempomap_segments(recs, *s, n_frames, index, segs); });
}
int mx_deck_tempomap_at(const mx_deck_tempo_segment* segs, uint32_t n, int64_t pos_q32, mx_deck_beats* grid, uint32_t* segment) {
    return guard([&] { mx::deck_tempomap_at(segs, n, pos_q32, grid, segment); });
}
int mx_deck_tempomap_step(const mx_deck_beats* grid, int64_t out_period_q32, int64_t* step_q32) {
    return guard([&] { REQUIRE(grid && step_q32, "NULL argument"); *step_q32 = mx::deck_tempomap_step(*grid, out_period_q32); });
}
int mx_deck_analyse_tempomap(mx_deck* d, const mx_deck_tempomap* s) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.tempomap.analyse(s); });
}
int mx_deck_read_tempomap(mx_deck* d, uint64_t first, uint64_t n, mx_deck_comb* dst) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.tempomap.read(first, n, dst); });
}
int mx_deck_read_tempomap_onsets(mx_deck* d, uint64_t first, uint64_t n, uint32_t* w) {
    return guard([&] { REQUIRE(d, "deck is NULL"); d->d.tempomap.read_onsets(first, n, w); });
}
int mx_deck_debug_last_tempomap(uint32_t out[4]) {
    return guard([&] { REQUIRE(out, "out is NULL"); mx::DeckTempoMap::debug_last(out); });
}
int mx_deck_waveform_check(const mx_deck_waveform* p) {
    return guard([&] { REQUIRE(p, "settings are NULL"); mx::deck_waveform_check(*p); });
}
int mx_deck_waveform_view(int64_t pos_q32, uint32_t frames_per_px, uint32_t playhead_x, int64_t* first_frame) {
    return guard([&] { REQUIRE(first_frame, "first_frame is NULL"); *first_frame = mx::deck_waveform_view(pos_q32, frames_per_px, playhead_x); });
}
int mx_deck_render_waveform(mx_deck* d, const mx_deck_waveform* p, mx_dframe** out, void* stream) {
    return guard([&] {
        REQUIRE(d && p && out, "NULL argument");
        mx::DFrame* f = d->d.columns.render_waveform(*p, mx::abi_video_stream(stream));   // (*out is written only once the launch is on the stream)
        *out = reinterpret_cast<mx_dframe*>(f);
    });
}
int mx_deck_waveform_host(const mx_deck_column* cols, uint64_t n_cols, uint32_t column, uint64_t n_frames, const mx_deck_waveform* p,
                          uint8_t* y, int32_t y_stride, uint8_t* u, uint8_t* v, int32_t c_stride) {
    return guard([&] { REQUIRE(p, "settings are NULL"); mx::deck_waveform_host(cols, n_cols, column, n_frames, *p, y, y_stride, u, v, c_stride); });
}
int mx_deck_debug_last_waveform(uint32_t out[4]) {
    return guard([&] { REQUIRE(out, "out is NULL"); mx::deck_debug_last_waveform(out); });
}

}  // extern "C"

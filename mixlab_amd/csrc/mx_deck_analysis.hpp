// mx_deck_analysis.hpp -- what the deck's whole-track analyses share (DESIGN.md section 0.17 "the shared protocol"): the free-or-grow step of analyse(settings),
// the checked window read, and the process-wide record of the last launch's forms.  An analysis is one subclass that holds its own state (mx_deck_columns.hpp,
// mx_deck_loudkey.hpp, mx_deck_finegrid.hpp) and one member of Deck (mx_deck.hpp); nobody iterates over them, so nothing here is virtual (internal).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

#include "mx_common.hpp"

namespace mx {

const uint64_t kDeckMaxFrames = (uint64_t)1 << 30;   // the longest track

// everything an analysis reads of its deck: the whole coupling.  Deck fills it once, in its constructor.
struct DeckTrack { const uint32_t* track = nullptr; uint64_t n_frames = 0; int device = -1; hipStream_t load_stream = nullptr; };

// forms[4] of the last launch that succeeded, of any deck of the process (mx_deck_debug_last_*): one per analysis class
class DeckLastForms {
public:
    void set(const uint32_t forms[4]);
    void get(uint32_t out[4]);
private:
    std::mutex mu_;
    uint32_t forms_[4] = {0u, 0u, 0u, 0u};
};

class DeckTrackAnalysis {
protected:
    // how a read names what it refuses, and its copy
    struct ReadNouns { const char* none; const char* beyond; const char* null_dst; const char* copy; };

    DeckTrackAnalysis(const DeckTrack& deck, DeckLastForms& last) : deck_(deck), last_(last) {}
    ~DeckTrackAnalysis() = default;
    // The first device step of analyse(settings), after the settings passed their check: results of need_bytes are coming, or (freeing) the results go.  The load
    // stream is waited for only when the buffer goes (freed, or too small) or force_wait says that something else an analysis in flight uses does; a buffer that is
    // large enough stays.  count_ is 0 from before anything that can throw until launched(): MX_ERR_NOMEM leaves the deck without the analysis.  false: freed, return.
    bool prepare(size_t need_bytes, bool freeing, bool force_wait = false);
    // ... and its last: the launch is checked, the results count, the forms are the process' last
    void launched(const char* what, uint64_t count, const uint32_t forms[4]);
    // items [first, first + n) of `limit` items of item_bytes each that start byte_offset into the buffer; cap_bytes: the room at dst, where the caller states it.
    // Refusals come in this order: no results, the window, the room, dst; n = 0 then returns without touching the device.
    void read_window(uint64_t first, uint64_t n, void* dst, size_t item_bytes, size_t byte_offset, uint64_t limit, const ReadNouns& w, size_t cap_bytes = SIZE_MAX);
    void wait_and_copy(void* dst, size_t byte_offset, size_t bytes, const char* what);   // the one wait for the load stream and the one copy of every read

    const DeckTrack& deck_;
    DevBuf buf_;            // the results, written on the load stream only
    uint64_t count_ = 0;    // ... in the unit the analysis counts them; 0: none, whatever else the subclass remembers
private:
    DeckLastForms& last_;
};

}  // namespace mx

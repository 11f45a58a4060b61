// mx_deck_analysis.cpp -- what the deck's whole-track analyses share (mx_deck_analysis.hpp; DESIGN.md section 0.17 "the shared protocol").
#include "mx_deck_analysis.hpp"

#include <cstring>

namespace mx {

void DeckLastForms::set(const uint32_t forms[4]) {
    std::lock_guard<std::mutex> lock(mu_);
    std::memcpy(forms_, forms, sizeof forms_);
}

void DeckLastForms::get(uint32_t out[4]) {
    std::lock_guard<std::mutex> lock(mu_);
    std::memcpy(out, forms_, sizeof forms_);
}

bool DeckTrackAnalysis::prepare(size_t need_bytes, bool freeing, bool force_wait) {
    hip_check(hipSetDevice(deck_.device), "hipSetDevice");
    const bool goes = freeing || buf_.bytes < need_bytes;
    if (goes || force_wait) {
        hip_check(hipStreamSynchronize(deck_.load_stream), "hipStreamSynchronize");   // an analysis in flight still uses what goes
        count_ = 0;
        if (goes) buf_.free_();
        if (freeing) return false;
        if (!buf_.p) buf_.alloc(need_bytes);   // (MX_ERR_NOMEM leaves the deck without this analysis)
    }
    count_ = 0;
    return true;
}

void DeckTrackAnalysis::launched(const char* what, uint64_t count, const uint32_t forms[4]) {
    hip_check(hipGetLastError(), what);
    count_ = count;
    last_.set(forms);
}

void DeckTrackAnalysis::read_window(uint64_t first, uint64_t n, void* dst, size_t item_bytes, size_t byte_offset, uint64_t limit, const ReadNouns& w, size_t cap_bytes) {
    if (!count_) throw Error(MX_ERR_INVALID, w.none);
    if (first > limit || n > limit - first) throw Error(MX_ERR_INVALID, w.beyond);
    if (cap_bytes / item_bytes < n) throw Error(MX_ERR_INVALID, "deck: cap_bytes is below n records");
    if (n && !dst) throw Error(MX_ERR_INVALID, w.null_dst);
    if (!n) return;
    wait_and_copy(dst, byte_offset + (size_t)first * item_bytes, (size_t)n * item_bytes, w.copy);
}

void DeckTrackAnalysis::wait_and_copy(void* dst, size_t byte_offset, size_t bytes, const char* what) {
    hip_check(hipSetDevice(deck_.device), "hipSetDevice");
    hip_check(hipStreamSynchronize(deck_.load_stream), "hipStreamSynchronize");
    hip_check(hipMemcpy(dst, (const char*)buf_.p + byte_offset, bytes, hipMemcpyDeviceToHost), what);
}

}  // namespace mx

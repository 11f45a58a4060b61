// mx_deck_columns.hpp -- the deck's band columns, onsets and their autocorrelation (include/mixlab_gpu.h "ANALYSIS"; mx_k_deck_analyse.hip):
// the host-only rule functions and the deck's first analysis (internal).
#pragma once
#include "mx_deck_analysis.hpp"

namespace mx {

struct DFrame;

void deck_analysis_check(const mx_deck_analysis& a);                                 // throws Error(MX_ERR_INVALID) naming the rule
void deck_analysis_bands(double rate, double f_lo, double f_hi, uint32_t taps, mx_deck_analysis& a);
uint64_t deck_column_count(uint64_t n_frames, uint32_t column);
void deck_columns_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_analysis& a, uint64_t first, uint64_t n, mx_deck_column* cols, uint64_t* R_or_null);
void deck_beatgrid(const mx_deck_column* cols, uint64_t n_cols, const uint64_t* R, uint32_t max_lag, uint32_t column, double rate, double bpm_lo, double bpm_hi, mx_deck_grid& out);

// one buffer -- columns (count_ x 56 bytes), R (lag_ x 8), onsets (count_ x 4)
class DeckColumns : public DeckTrackAnalysis {
public:
    explicit DeckColumns(const DeckTrack& deck);
    ~DeckColumns();
    void analyse(const mx_deck_analysis* a);                               // NULL: frees the results.  Asynchronous on the load stream.
    void read_columns(uint64_t first, uint64_t n, mx_deck_column* dst);    // waits for the analysis
    void read_autocorr(uint64_t* R, uint32_t cap);                         // waits for the analysis
    static void debug_last(uint32_t out[4]);
    // The waveform picture of the records (mx_deck_waveform.cpp; include/mixlab_gpu.h "WAVEFORM"): a new frame with one reference, launched on s behind analysed_,
    // with no host wait.  rendered_ follows the last render on its stream: analyse() makes the load stream wait for it before the records are rewritten or go.
    DFrame* render_waveform(const mx_deck_waveform& p, hipStream_t s);
private:
    uint32_t lag_ = 0;
    uint32_t column_ = 0;
    hipEvent_t analysed_ = nullptr;   // behind the last analysis on the load stream (created by the first analysis)
    hipEvent_t rendered_ = nullptr;   // behind the last render on its stream (created by the first render)
};

}  // namespace mx

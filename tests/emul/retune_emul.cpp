// Host build of the retune lane code (csrc/retune_core.hpp): the per-channel resets run lane by lane as the kernels of tetra_retune.hip
// run them (one 64-lane group per listed channel), and the history ring's keep / rebuild element by element.  TEST TOOL.
#include <cstdint>

#include "../../sdrpp-tetra-demodulator_amd/csrc/retune_core.hpp"

extern "C" {

int retune_emul_view_bytes(void) { return (int)sizeof(retune::DemodView); }

void retune_emul_reset_demod(const retune::DemodView* v, const int32_t* channels, int n, int lanes) {
    for (int b = 0; b < n; b++)
        for (int lane = lanes - 1; lane >= 0; lane--) retune::reset_demod_channel(*v, channels[b], lane, lanes);
}

void retune_emul_reset_tail(uint32_t* state, int state_words, uint32_t* carry, int carry_words, uint32_t* cell, int cell_words,
                            const int32_t* channels, int n, int lanes) {
    const retune::CellView none = { nullptr, 0 };          // a chain without link figures, miss counters and hand-over fields
    const retune::TailView tv = { { state, carry, state_words, carry_words }, { cell, cell_words }, none, none, none };
    for (int b = 0; b < n; b++)
        for (int lane = lanes - 1; lane >= 0; lane--) retune::reset_tail_channel(tv, channels[b], lane, lanes);
}

// one call's share of the ring: x [n_in][M] complex64 after n0 earlier frames
void retune_emul_keep(const float* x, int M, long long n0, int n_in, int hist, float* ring) {
    const int rows = n_in < hist ? n_in : hist;
    for (long long i = (long long)rows * M - 1; i >= 0; i--) retune::keep_element(x, M, n0, n_in, rows, hist, i, ring);
}

// the delay-line columns of the listed slots: line [hist][C] complex64
void retune_emul_rebuild(const float* ring, int M, int hist, long long n_total, const int32_t* slots, const int32_t* bins, int n, int C, float* line) {
    for (int r = 0; r < hist; r++)
        for (int j = 0; j < n; j++) retune::rebuild_element(ring, M, hist, n_total, r, bins[j], slots[j], C, line);
}

}  // extern "C"

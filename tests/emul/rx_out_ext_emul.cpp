// Host build of the extras writer's lane code (csrc/rx_out_core.hpp: ext_stage / ext_store / table_copy / layout_ext), run thread by
// thread as k_out_ext_write of tetra_rx_out.hip runs it: per tile of kTile rows the kept rows are ranked, the column is staged in the
// tile's "LDS" and stored as one contiguous run.  The ranking itself (compact_core::block_rank, a ballot) is stated here as what it
// computes: the kept rows before a row.  TEST TOOL.
#include <cstdint>
#include <cstring>

#define TETRA_HOST_EMUL 1
#include "../../sdrpp-tetra-demodulator_amd/csrc/rx_out_core.hpp"

namespace {
constexpr int kTile = 128;

// one column of n rows (element of row j at col + j * stride) -> dst, whose column starts at byte col_off and whose first output row
// is first_row (the tiles' first output rows follow from the kept counts, as the scan leaves them)
template <int ESZ> void write_column(const uint8_t* col, size_t stride, const int32_t* ok, int n, int crc, uint64_t col_off, int first_row, uint8_t* dst) {
    int base = first_row;
    for (int t0 = 0; t0 < n; t0 += kTile) {
        alignas(16) uint8_t lds[16 + kTile * 4];
        std::memset(lds, 0xEE, sizeof(lds));          // (the bytes of a chunk outside the run are never stored)
        uint8_t src[kTile];
        int cnt = 0;
        for (int t = 0; t < kTile; t++)
            if (t0 + t < n && (!crc || ok[t0 + t] != 0)) src[cnt++] = (uint8_t)t;
        const uint64_t b0 = col_off + (uint64_t)ESZ * (uint64_t)base;
        for (int t = kTile - 1; t >= 0; t--) rx_out::ext_stage<ESZ>(lds, b0, col, stride, t0, src, cnt, t, kTile);      // (barrier)
        for (int t = kTile - 1; t >= 0; t--) rx_out::ext_store<ESZ>(dst, b0, lds, cnt, t, kTile);
        base += cnt;
    }
}
}  // namespace

extern "C" {

// elem = 4: col is uint32 [n]; elem = 1: col is [n][stride] bytes and the element is byte `at` of a row
void rx_out_ext_emul_column(const uint8_t* col, int elem, int stride, int at, const int32_t* ok, int n, int crc, uint64_t col_off, int first_row,
                            uint8_t* dst) {
    if (elem == 4) write_column<4>(col, 4, ok, n, crc, col_off, first_row, dst);
    else write_column<1>(col + at, (size_t)stride, ok, n, crc, col_off, first_row, dst);
}

// a per-channel table as the launch copies it: `groups` workgroups of kTile threads
void rx_out_ext_emul_table(const uint8_t* src, uint64_t bytes, int groups, uint8_t* dst) {
    for (int g = groups - 1; g >= 0; g--)
        for (int t = kTile - 1; t >= 0; t--) rx_out::table_copy(dst, src, bytes, (uint64_t)g * kTile + (uint64_t)t, (uint64_t)groups * kTile);
}

// the layouts: classic header and extension header of kinds kind[0 .. n) with n_rows[] rows; returns the total
uint64_t rx_out_ext_emul_layout(const int* kind, const int* n_rows, int n, int flags, int extras, int n_channels, tetra_rx_out_header_t* hd,
                                tetra_rx_out_ext_header_t* ex) {
    const uint64_t classic = rx_out::layout(hd, kind, n_rows, n_rows, n, flags);
    return rx_out::layout_ext(ex, kind, n_rows, n, classic, extras, n_channels);
}

uint64_t rx_out_ext_emul_snap_offset(int tab, int n_channels) { return rx_out::snap_offset(tab, n_channels); }

}  // extern "C"

// san_rx_out_ext.cpp -- the host side of an extended delivery (csrc/rx_out_core.hpp: layout_ext, tetra_rx_out_view_ext,
// tetra_rx_out_view_channels, and the extras writer's lane code) under AddressSanitizer + UBSan (TEST TOOL, no GPU).  Builds extended
// deliveries to the documented layout with the writer's own lane code, then reads them back from heap blocks of exactly the size
// given -- truncated at every length, and with every 4-byte word of both headers flipped -- so that any access outside a buffer is a
// report.  Every case must be refused or hand out views inside the buffer.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define TETRA_HOST_EMUL 1
#include "../../sdrpp-tetra-demodulator_amd/csrc/rx_out_core.hpp"

static int fail(const char* what, long long v) { std::fprintf(stderr, "san_rx_out_ext: %s (%lld)\n", what, v); return 1; }

constexpr int kTile = 128;
static const int kChannels = 5;

// 16-byte aligned heap block of exactly `len` bytes (ASan guards both ends)
static unsigned char* block(size_t len) {
    void* p = nullptr;
    if (posix_memalign(&p, 16, len ? len : 1) != 0) std::abort();
    return static_cast<unsigned char*>(p);
}

// every kind, n_rows[k] rows, all rows kept; the columns written tile by tile by the lane code, the tables by table_copy
static std::vector<unsigned char> make(const int* n_rows, int flags, int extras, size_t* ext_at) {
    int kind[TETRA_RX_N_KINDS];
    for (int k = 0; k < TETRA_RX_N_KINDS; k++) kind[k] = k;
    tetra_rx_out_header_t hd;
    tetra_rx_out_ext_header_t ex;
    std::memset(&hd, 0, sizeof(hd));
    std::memset(&ex, 0, sizeof(ex));
    const uint64_t classic = rx_out::layout(&hd, kind, n_rows, n_rows, TETRA_RX_N_KINDS, flags);
    const uint64_t total = rx_out::layout_ext(&ex, kind, n_rows, TETRA_RX_N_KINDS, classic, extras, kChannels);
    hd.magic = TETRA_RX_OUT_MAGIC;
    hd.status = TETRA_OK;
    hd.flags = flags;
    hd.call = ex.call = 7;
    ex.magic = TETRA_RX_OUT_EXT_MAGIC;
    unsigned char* dst = block(total);
    std::memset(dst, 0, total);
    std::memcpy(dst, &hd, sizeof(hd));
    *ext_at = (size_t)rx_out::align16(classic);
    std::memcpy(dst + *ext_at, &ex, sizeof(ex));
    for (int k = 0; k < TETRA_RX_N_KINDS; k++) {
        const int n = n_rows[k];
        uint32_t* col = static_cast<uint32_t*>(std::malloc(sizeof(uint32_t) * (size_t)(n ? n : 1)));      // exact-size sources
        unsigned char* t2 = static_cast<unsigned char*>(std::malloc((size_t)(n ? n : 1) * 32));
        for (int r = 0; r < n; r++) { col[r] = (uint32_t)(r * 2654435761u + (uint32_t)k); t2[(size_t)r * 32 + 30] = (unsigned char)(r * 7 + k); }
        const uint64_t off[3] = { ex.kinds[k].biterr_offset, ex.kinds[k].rank_offset, ex.kinds[k].aach_dist_offset };
        for (int t0 = 0; t0 < n; t0 += kTile) {
            alignas(16) uint8_t lds[16 + kTile * 4];
            uint8_t src[kTile];
            const int cnt = n - t0 < kTile ? n - t0 : kTile;
            for (int t = 0; t < cnt; t++) src[t] = (uint8_t)t;
            for (int c = 0; c < 3; c++) {
                if (!off[c]) continue;
                const uint64_t b0 = off[c] + (uint64_t)rx_out::row_elem_bytes(c) * (uint64_t)t0;
                for (int t = 0; t < kTile; t++) {
                    if (c < 2) rx_out::ext_stage<4>(lds, b0, reinterpret_cast<const uint8_t*>(col), 4, t0, src, cnt, t, kTile);
                    else rx_out::ext_stage<1>(lds, b0, t2 + 30, 32, t0, src, cnt, t, kTile);
                }
                for (int t = 0; t < kTile; t++) {
                    if (c < 2) rx_out::ext_store<4>(dst, b0, lds, cnt, t, kTile);
                    else rx_out::ext_store<1>(dst, b0, lds, cnt, t, kTile);
                }
            }
        }
        std::free(col);
        std::free(t2);
    }
    const uint64_t tab[4] = { ex.cell_offset, ex.sync_state_offset, ex.sync_misses_offset, ex.link_offset };
    for (int j = 0; j < 4; j++) {
        if (!tab[j]) continue;
        const size_t bytes = (size_t)rx_out::chan_elem_bytes(j) * kChannels;
        unsigned char* src = block(bytes);
        for (size_t i = 0; i < bytes; i++) src[i] = (unsigned char)(i * 13 + j);
        for (int t = 0; t < 2 * kTile; t++) rx_out::table_copy(dst + tab[j], src, bytes, (uint64_t)t, 2 * kTile);
        if (std::memcmp(dst + tab[j], src, bytes) != 0) std::abort();
        std::free(src);
    }
    std::vector<unsigned char> out(dst, dst + total);
    std::free(dst);
    return out;
}

// every kind through both readers from an exact-size copy of the first `len` bytes, touching every byte they hand out; the first
// status that is not OK
static int read_all(const std::vector<unsigned char>& full, size_t len) {
    unsigned char* p = block(len);
    std::memcpy(p, full.data(), len);
    int first = TETRA_OK;
    volatile unsigned sum = 0;
    for (int k = 0; k < TETRA_RX_N_KINDS; k++) {
        const uint32_t* be = nullptr;
        const int32_t* rk = nullptr;
        const uint8_t* ad = nullptr;
        int n = 0;
        const int rc = rx_out::view_ext(p, len, k, &be, &rk, &ad, &n);
        if (rc != TETRA_OK) { if (first == TETRA_OK) first = rc; continue; }
        for (int r = 0; r < n; r++) sum += (be ? be[r] : 0u) + (rk ? (unsigned)rk[r] : 0u) + (ad ? ad[r] : 0u);
    }
    const tetra_lmac_cell_state_t* cell = nullptr;
    const tetra_bsync_state_t* st = nullptr;
    const int32_t* miss = nullptr;
    const tetra_rx_link_t* link = nullptr;
    int nc = 0;
    const int rc = rx_out::view_channels(p, len, &cell, &st, &miss, &link, &nc);
    if (rc != TETRA_OK) { if (first == TETRA_OK) first = rc; }
    else
        for (int c = 0; c < nc; c++)
            sum += (cell ? cell[c].phy_mn + cell[c].scramb_init : 0u) + (st ? st[c].next_frame_start_bitnum : 0u) + (miss ? (unsigned)miss[c] : 0u) +
                   (link ? (unsigned)link[c].bits + link[c].blocks_crc_bad : 0u);
    (void)sum;
    std::free(p);
    return first;
}

int main() {
    const int rows[TETRA_RX_N_KINDS] = { 5, 129, 3, 0, 9, 11 };
    for (int flags = 0; flags < 4; flags++) {
        for (int extras : { 247, 1 | 64, 4 | 16, 2 }) {
            size_t ext_at = 0;
            const std::vector<unsigned char> buf = make(rows, flags, extras, &ext_at);
            if (read_all(buf, buf.size()) != TETRA_OK) return fail("whole buffer", extras);
            for (size_t len = 0; len < buf.size(); len++)
                if (read_all(buf, len) == TETRA_OK) return fail("truncated buffer accepted", (long long)len);
            // every 4-byte word of both headers flipped in turn: refused, or still views inside the buffer (ASan watches)
            for (size_t h0 : { (size_t)0, ext_at }) {
                const size_t hlen = h0 ? sizeof(tetra_rx_out_ext_header_t) : sizeof(tetra_rx_out_header_t);
                for (size_t at = 0; at + 4 <= hlen; at += 4)
                    for (uint32_t v : { 0xffffffffu, 0x7fffffffu, 0x80000000u, 1u, 16u, 0xfffffff0u }) {
                        std::vector<unsigned char> bad = buf;
                        std::memcpy(bad.data() + h0 + at, &v, 4);
                        (void)read_all(bad, bad.size());
                    }
            }
            // a classic-only buffer has no extension block
            if (read_all(buf, (size_t)reinterpret_cast<const tetra_rx_out_header_t*>(buf.data())->bytes) != TETRA_ERR_UNSUPPORTED) return fail("classic only", extras);
            std::vector<unsigned char> bad = buf;
            bad[ext_at] ^= 1;
            if (read_all(bad, bad.size()) != TETRA_ERR_ARG) return fail("extension magic", extras);
        }
    }
    std::printf("san_rx_out_ext: ok\n");
    return 0;
}

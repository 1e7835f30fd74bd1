// rx_out_core.hpp -- the arithmetic of a delivery (include/tetra_rx_out.h): row widths, the buffer layout, bit packing, and the
// host-side reader / unpacker.  Shared by the delivery kernels (tetra_rx_out.hip) and host builds (the sanitizer driver), like the
// other *_core.hpp files; the reader and the unpacker are host code only.  Below them the same for the extension block
// (include/ext/tetra_rx_out_ext.h): its layout, the extras writer's lane code, its readers.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/ext/tetra_rx_out_ext.h"
#include "../../include/tetra_rx_out.h"

#if defined(__HIPCC__) && !defined(TETRA_HOST_EMUL)
#define RXO_FN __host__ __device__ __forceinline__
#else
#define RXO_FN static inline
#endif

namespace rx_out {

constexpr uint64_t kHeaderBytes = sizeof(tetra_rx_out_header_t);
constexpr int kFlagsAll = TETRA_RX_OUT_PACKED | TETRA_RX_OUT_CRC_GOOD;
static_assert(kHeaderBytes == 224 && kHeaderBytes % 16 == 0, "the header is 14 16-byte words");
static_assert(sizeof(tetra_rx_block_t) == 24, "labels are 24 bytes");

RXO_FN int type1_bits(int kind) {
    switch (kind) {
    case TETRA_RX_KIND_SB1: return 60;
    case TETRA_RX_KIND_BBK: return 30;
    case TETRA_RX_KIND_SB2:
    case TETRA_RX_KIND_NDB1:
    case TETRA_RX_KIND_NDB2: return 124;
    case TETRA_RX_KIND_SCH_F: return 268;
    default: return -1;
    }
}
// bytes per type-1 row: one per bit, or packed 8 per byte (8 / 4 / 16 / 16 / 16 / 34)
RXO_FN int row_bytes(int kind, int flags) {
    const int nb = type1_bits(kind);
    return (flags & TETRA_RX_OUT_PACKED) ? (nb + 7) >> 3 : nb;
}
RXO_FN uint64_t align16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }
// Padding a kind's sections can add beyond their rows: up to 15 bytes before the labels, 8 before the bits (labels are 24 bytes each).
constexpr uint64_t kPadPerKind = 24;

// Fills hd's kinds[0 .. n) for the kinds kind[0 .. n) (ascending) with rows n_rows[i] of n_dec[i] and returns the bytes the
// delivery needs.  magic / status / flags / call are the caller's.
RXO_FN uint64_t layout(tetra_rx_out_header_t* hd, const int* kind, const int* n_rows, const int* n_dec, int n, int flags) {
    uint64_t off = kHeaderBytes;
    hd->n_kinds = n;
    for (int i = 0; i < TETRA_RX_N_KINDS; i++) {
        tetra_rx_out_kind_t& e = hd->kinds[i];
        if (i >= n) {
            e.kind = e.n_rows = e.n_rows_decoded = e.row_bytes = 0;
            e.blocks_offset = e.bits_offset = 0;
            continue;
        }
        e.kind = kind[i];
        e.n_rows = n_rows[i];
        e.n_rows_decoded = n_dec[i];
        e.row_bytes = row_bytes(kind[i], flags);
        e.blocks_offset = align16(off);
        e.bits_offset = align16(e.blocks_offset + sizeof(tetra_rx_block_t) * (uint64_t)n_rows[i]);
        off = e.bits_offset + (uint64_t)e.row_bytes * (uint64_t)n_rows[i];
    }
    hd->bytes = off;
    return off;
}

// One packed byte from eight bit bytes (0 / 1, the first bit in the lowest byte of v): the first bit in bit 7; bits at or past
// `valid` are zero (a row's padding).
RXO_FN uint32_t pack8(uint64_t v, int valid) {
    uint32_t r = 0;
    for (int i = 0; i < 8; i++)
        if (i < valid) r |= (uint32_t)((v >> (8 * i)) & 1u) << (7 - i);
    return r;
}

// ---- host side ----

inline int view(const void* buf, uint64_t bytes, int kind, const tetra_rx_block_t** blocks, const uint8_t** bits, int* n_rows,
                int* row_bytes_out) {
    if (!buf || kind < 0 || kind >= TETRA_RX_N_KINDS || bytes < kHeaderBytes) return TETRA_ERR_ARG;
    tetra_rx_out_header_t hd;
    memcpy(&hd, buf, sizeof(hd));
    if (hd.magic != TETRA_RX_OUT_MAGIC) return TETRA_ERR_ARG;
    if (hd.status != TETRA_OK) return hd.status < 0 ? hd.status : TETRA_ERR_ARG;
    if ((hd.flags & ~kFlagsAll) || hd.n_kinds < 0 || hd.n_kinds > TETRA_RX_N_KINDS || hd.bytes < kHeaderBytes || hd.bytes > bytes)
        return TETRA_ERR_ARG;
    for (int i = 0; i < hd.n_kinds; i++) {
        const tetra_rx_out_kind_t& e = hd.kinds[i];
        if (e.kind != kind) continue;
        if (e.n_rows < 0 || e.n_rows_decoded < e.n_rows || e.row_bytes != row_bytes(kind, hd.flags)) return TETRA_ERR_ARG;
        const uint64_t n = (uint64_t)e.n_rows;
        // both sections after the header and inside hd.bytes (which is inside the buffer); no product can overflow: n < 2^31
        if (e.blocks_offset < kHeaderBytes || e.blocks_offset > hd.bytes || e.blocks_offset % 16 ||
            n * sizeof(tetra_rx_block_t) > hd.bytes - e.blocks_offset)
            return TETRA_ERR_ARG;
        if (e.bits_offset < kHeaderBytes || e.bits_offset > hd.bytes || e.bits_offset % 16 || n * (uint64_t)e.row_bytes > hd.bytes - e.bits_offset)
            return TETRA_ERR_ARG;
        const uint8_t* base = static_cast<const uint8_t*>(buf);
        if ((uintptr_t)(base + e.blocks_offset) % alignof(tetra_rx_block_t)) return TETRA_ERR_ALIGN;
        if (blocks) *blocks = reinterpret_cast<const tetra_rx_block_t*>(base + e.blocks_offset);
        if (bits) *bits = base + e.bits_offset;
        if (n_rows) *n_rows = e.n_rows;
        if (row_bytes_out) *row_bytes_out = e.row_bytes;
        return TETRA_OK;
    }
    return TETRA_ERR_UNSUPPORTED;
}

inline int unpack_bits(const uint8_t* packed, int n_rows, int rb, int n_bits, uint8_t* out, int out_stride) {
    if (n_rows < 0 || rb < 0 || n_bits < 0 || (long long)n_bits > 8LL * rb) return TETRA_ERR_ARG;
    if (n_rows > 0 && (!packed || !out)) return TETRA_ERR_ARG;
    if (out_stride < n_bits) return TETRA_ERR_SIZE;
    for (int r = 0; r < n_rows; r++) {
        const uint8_t* p = packed + (size_t)r * (size_t)rb;
        uint8_t* o = out + (size_t)r * (size_t)out_stride;
        for (int i = 0; i < n_bits; i++) o[i] = (uint8_t)((p[i >> 3] >> (7 - (i & 7))) & 1u);
    }
    return TETRA_OK;
}

// ---- the extension block (include/ext/tetra_rx_out_ext.h) ----

constexpr int kExtrasRow = TETRA_RX_OUT_EXT_ROW_ALL, kExtrasChan = TETRA_RX_OUT_EXT_CHAN_ALL, kExtrasAll = kExtrasRow | kExtrasChan;
constexpr uint64_t kExtHeaderBytes = sizeof(tetra_rx_out_ext_header_t);
static_assert(kExtHeaderBytes == 256 && sizeof(tetra_rx_out_ext_kind_t) == 32, "the extension header is 16 16-byte words");
static_assert(sizeof(tetra_lmac_cell_state_t) == 40 && sizeof(tetra_bsync_state_t) == 16 && sizeof(tetra_rx_link_t) == 24, "the per-channel tables");

// the row extras in column order, the channel extras in table order
constexpr int kRowCols = 3, kChanTables = 4;
RXO_FN int row_extra(int col) { return col == 0 ? TETRA_RX_OUT_EXT_ROW_BITERR : col == 1 ? TETRA_RX_OUT_EXT_ROW_LIST_RANK : TETRA_RX_OUT_EXT_ROW_AACH_DIST; }
RXO_FN int row_elem_bytes(int col) { return col == 2 ? 1 : 4; }
// the coded kinds have the first two columns, the AACH the third
RXO_FN bool kind_has(int kind, int col) { return (col == 2) == (kind == TETRA_RX_KIND_BBK); }
RXO_FN int chan_extra(int tab) { return TETRA_RX_OUT_EXT_CHAN_CELL << tab; }
RXO_FN int chan_elem_bytes(int tab) {
    return (int)(tab == 0 ? sizeof(tetra_lmac_cell_state_t) : tab == 1 ? sizeof(tetra_bsync_state_t) : tab == 2 ? sizeof(int32_t) : sizeof(tetra_rx_link_t));
}
// A handle's snapshot of one call: the four tables one after the other, each 16-byte aligned, whatever the armed mask
RXO_FN uint64_t snap_offset(int tab, int n_channels) {
    uint64_t off = 0;
    for (int i = 0; i < tab; i++) off = align16(off + (uint64_t)chan_elem_bytes(i) * (uint64_t)n_channels);
    return off;
}
RXO_FN uint64_t snap_bytes(int n_channels) { return snap_offset(kChanTables, n_channels); }

// Fills *ex for a delivery whose classic part holds kind[0 .. n) with n_rows[i] rows in classic_bytes bytes, and returns the bytes of
// the whole buffer contents.  magic / call are the caller's.
RXO_FN uint64_t layout_ext(tetra_rx_out_ext_header_t* ex, const int* kind, const int* n_rows, int n, uint64_t classic_bytes, int extras,
                           int n_channels) {
    uint64_t end = align16(classic_bytes) + kExtHeaderBytes;
    int got = extras & kExtrasChan;
    ex->n_channels = n_channels;
    ex->n_kinds = n;
    for (int i = 0; i < TETRA_RX_N_KINDS; i++) {
        tetra_rx_out_ext_kind_t& e = ex->kinds[i];
        e.kind = i < n ? kind[i] : 0;
        e.n_rows = i < n ? n_rows[i] : 0;
        uint64_t at[kRowCols] = { 0, 0, 0 };
        for (int c = 0; c < kRowCols; c++) {
            if (i >= n || !(extras & row_extra(c)) || !kind_has(kind[i], c)) continue;
            at[c] = align16(end);
            end = at[c] + (uint64_t)row_elem_bytes(c) * (uint64_t)n_rows[i];
            got |= row_extra(c);
        }
        e.biterr_offset = at[0];
        e.rank_offset = at[1];
        e.aach_dist_offset = at[2];
    }
    uint64_t tab[kChanTables] = { 0, 0, 0, 0 };
    for (int t = 0; t < kChanTables; t++) {
        if (!(extras & chan_extra(t))) continue;
        tab[t] = align16(end);
        end = tab[t] + (uint64_t)chan_elem_bytes(t) * (uint64_t)n_channels;
    }
    ex->cell_offset = tab[0];
    ex->sync_state_offset = tab[1];
    ex->sync_misses_offset = tab[2];
    ex->link_offset = tab[3];
    ex->extras = got;
    ex->bytes = end;
    return end;
}

// The extras writer's lane code (k_out_ext_write; tests/emul/rx_out_ext_emul.cpp runs it on the host).  A tile's share of one column
// is ONE contiguous run of the output: cnt elements of ESZ bytes from output byte b0 on.  It is staged so that lds[16 c .. 16 c + 16)
// is the 16-byte aligned chunk c of the output (the run starts at lds[b0 & 15]) and then stored with 16-byte stores of the whole
// chunks and ESZ-byte stores at the two ends -- the scheme of k_out_write's labels.  The column starts 16-byte aligned, so b0 is a
// multiple of ESZ.  src[r] = the tile-local row of the r-th kept row; the element of row j is at col + j * stride.
// N aligned bytes as one access (a 16-byte one is the store the scheme is about)
template <int N> RXO_FN void copy_aligned(uint8_t* d, const uint8_t* s) {
    __builtin_memcpy(__builtin_assume_aligned(d, N), __builtin_assume_aligned(s, N), N);
}
template <int ESZ>
RXO_FN void ext_stage(uint8_t* lds, uint64_t b0, const uint8_t* col, size_t stride, int t0, const uint8_t* src, int cnt, int t, int nt) {
    const int shift = (int)(b0 & 15);
    for (int r = t; r < cnt; r += nt) {
        const uint8_t* p = col + (size_t)(t0 + src[r]) * stride;
        copy_aligned<ESZ>(lds + shift + ESZ * r, p);
    }
}
template <int ESZ>
RXO_FN void ext_store(uint8_t* dst, uint64_t b0, const uint8_t* lds, int cnt, int t, int nt) {
    const int shift = (int)(b0 & 15), end = shift + ESZ * cnt;
    uint8_t* out = dst + (b0 - (uint64_t)shift);
    for (int c = t; 16 * c < end; c += nt) {
        if (16 * c >= shift && 16 * c + 16 <= end) {
            copy_aligned<16>(out + 16 * c, lds + 16 * c);
        } else {
            for (int j = 16 * c; j < 16 * c + 16; j += ESZ)
                if (j >= shift && j < end) copy_aligned<ESZ>(out + j, lds + j);
        }
    }
}
// a per-channel table (a multiple of 4 bytes, source and destination 16-byte aligned): 16-byte units i, i + n_units, ..., 4-byte words at the end
RXO_FN void table_copy(uint8_t* dst, const uint8_t* src, uint64_t bytes, uint64_t i, uint64_t n_units) {
    for (uint64_t c = i; 16 * c < bytes; c += n_units) {
        if (16 * c + 16 <= bytes) {
            copy_aligned<16>(dst + 16 * c, src + 16 * c);
        } else {
            for (uint64_t j = 16 * c; j < bytes; j += 4) copy_aligned<4>(dst + j, src + j);
        }
    }
}

// ---- host side of the extension block ----

// the extension header of a delivery whose classic part rx_out::view accepts; TETRA_OK and *ex, *hd filled, or a status
inline int ext_header(const void* buf, uint64_t bytes, tetra_rx_out_header_t* hd, tetra_rx_out_ext_header_t* ex) {
    if (!buf || bytes < kHeaderBytes) return TETRA_ERR_ARG;
    memcpy(hd, buf, sizeof(*hd));
    if (hd->magic != TETRA_RX_OUT_MAGIC) return TETRA_ERR_ARG;
    if (hd->status != TETRA_OK) return hd->status < 0 ? hd->status : TETRA_ERR_ARG;
    if ((hd->flags & ~kFlagsAll) || hd->n_kinds < 0 || hd->n_kinds > TETRA_RX_N_KINDS || hd->bytes < kHeaderBytes || hd->bytes > bytes) return TETRA_ERR_ARG;
    const uint64_t at = align16(hd->bytes);
    if (at > bytes || bytes - at < kExtHeaderBytes) return TETRA_ERR_UNSUPPORTED;      // the buffer ends before an extension header could
    memcpy(ex, static_cast<const uint8_t*>(buf) + at, sizeof(*ex));
    if (ex->magic != TETRA_RX_OUT_EXT_MAGIC || (ex->extras & ~kExtrasAll) || ex->call != hd->call || ex->n_kinds != hd->n_kinds || ex->n_channels < 0 ||
        ex->bytes < at + kExtHeaderBytes || ex->bytes > bytes)
        return TETRA_ERR_ARG;
    return TETRA_OK;
}
// a section of `count` elements of `elem` bytes at `off`: behind the extension header, inside ex.bytes, 16-byte aligned
inline bool ext_section_ok(const tetra_rx_out_header_t& hd, const tetra_rx_out_ext_header_t& ex, uint64_t off, uint64_t count, uint64_t elem) {
    const uint64_t first = align16(hd.bytes) + kExtHeaderBytes;
    return off >= first && off <= ex.bytes && off % 16 == 0 && count * elem <= ex.bytes - off;      // (count < 2^31, elem <= 40)
}

inline int view_ext(const void* buf, uint64_t bytes, int kind, const uint32_t** biterr, const int32_t** rank, const uint8_t** aach_dist, int* n_rows) {
    if (kind < 0 || kind >= TETRA_RX_N_KINDS) return TETRA_ERR_ARG;
    int n = 0;
    const int rc = view(buf, bytes, kind, nullptr, nullptr, &n, nullptr);      // the classic part, this kind's entry included
    if (rc != TETRA_OK) return rc;
    tetra_rx_out_header_t hd;
    tetra_rx_out_ext_header_t ex;
    const int rx = ext_header(buf, bytes, &hd, &ex);
    if (rx != TETRA_OK) return rx;
    for (int i = 0; i < hd.n_kinds; i++) {
        if (hd.kinds[i].kind != kind) continue;
        const tetra_rx_out_ext_kind_t& e = ex.kinds[i];
        if (e.kind != kind || e.n_rows != n) return TETRA_ERR_ARG;
        const uint64_t off[kRowCols] = { e.biterr_offset, e.rank_offset, e.aach_dist_offset };
        const uint8_t* at[kRowCols] = { nullptr, nullptr, nullptr };
        for (int c = 0; c < kRowCols; c++) {
            if (!off[c]) continue;
            if (!(ex.extras & row_extra(c)) || !kind_has(kind, c) || !ext_section_ok(hd, ex, off[c], (uint64_t)n, (uint64_t)row_elem_bytes(c))) return TETRA_ERR_ARG;
            at[c] = static_cast<const uint8_t*>(buf) + off[c];
            if ((uintptr_t)at[c] % (size_t)row_elem_bytes(c)) return TETRA_ERR_ALIGN;
        }
        if (biterr) *biterr = reinterpret_cast<const uint32_t*>(at[0]);
        if (rank) *rank = reinterpret_cast<const int32_t*>(at[1]);
        if (aach_dist) *aach_dist = at[2];
        if (n_rows) *n_rows = n;
        return TETRA_OK;
    }
    return TETRA_ERR_UNSUPPORTED;
}

inline int view_channels(const void* buf, uint64_t bytes, const tetra_lmac_cell_state_t** cell, const tetra_bsync_state_t** sync, const int32_t** misses,
                         const tetra_rx_link_t** link, int* n_channels) {
    tetra_rx_out_header_t hd;
    tetra_rx_out_ext_header_t ex;
    const int rc = ext_header(buf, bytes, &hd, &ex);
    if (rc != TETRA_OK) return rc;
    const uint64_t off[kChanTables] = { ex.cell_offset, ex.sync_state_offset, ex.sync_misses_offset, ex.link_offset };
    const uint8_t* at[kChanTables] = { nullptr, nullptr, nullptr, nullptr };
    for (int t = 0; t < kChanTables; t++) {
        if (!off[t]) continue;
        if (!(ex.extras & chan_extra(t)) || !ext_section_ok(hd, ex, off[t], (uint64_t)ex.n_channels, (uint64_t)chan_elem_bytes(t))) return TETRA_ERR_ARG;
        at[t] = static_cast<const uint8_t*>(buf) + off[t];
        if ((uintptr_t)at[t] % 8) return TETRA_ERR_ALIGN;
    }
    if (cell) *cell = reinterpret_cast<const tetra_lmac_cell_state_t*>(at[0]);
    if (sync) *sync = reinterpret_cast<const tetra_bsync_state_t*>(at[1]);
    if (misses) *misses = reinterpret_cast<const int32_t*>(at[2]);
    if (link) *link = reinterpret_cast<const tetra_rx_link_t*>(at[3]);
    if (n_channels) *n_channels = ex.n_channels;
    return TETRA_OK;
}

}  // namespace rx_out

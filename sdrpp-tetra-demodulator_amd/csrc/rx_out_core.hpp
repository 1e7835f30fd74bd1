// rx_out_core.hpp -- the arithmetic of a delivery (include/tetra_rx_out.h): row widths, the buffer layout, bit packing, and the
// host-side reader / unpacker.  Shared by the delivery kernels (tetra_rx_out.hip) and host builds (the sanitizer driver), like the
// other *_core.hpp files; the reader and the unpacker are host code only.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

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

}  // namespace rx_out

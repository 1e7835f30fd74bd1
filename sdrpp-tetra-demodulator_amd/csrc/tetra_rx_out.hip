// tetra_rx_out.hip -- a receive-chain call's decoded blocks delivered to the host in one asynchronous step (include/tetra_rx_out.h).
//
// Row counts exist only on the device, so the host cannot size a copy when it enqueues; the kernels write the delivery themselves,
// straight into the destination (mapped page-locked host memory or device memory).  Per delivery, on the handle's fetch stream behind
// the tail of the call it reads:
//
//   k_out_count   (CRC-good only)  per kind and tile of kTile rows: the rows with crc_ok != 0
//   k_out_layout  ONE workgroup: per kind the tiles' first output rows (a scan of the counts, in place), the layout, the header -> dst
//   k_out_write   per kind and tile: the kept rows' labels and type-1 rows (byte per bit or packed), compacted in LDS so that
//                 the tile's output is two contiguous runs, then written with 16-byte stores
// The count, the scan and the ranking of a tile's kept rows are the chain's one compaction (compact_core.hpp).
//
// No workgroup reads what another workgroup of the same launch writes (the per-XCD L2s are not coherent); every hand-over is a
// kernel boundary on one stream.  Nothing is written outside [dst, dst + capacity): the layout launch checks the size first, and a
// delivery that does not fit gets only its header.  The opt-in extension block (include/ext/tetra_rx_out_ext.h) adds two launches of
// its own around k_out_write (see below); without extras the three kernels above are all that is launched.
#include <hip/hip_runtime.h>

#include "../../include/ext/tetra_rx_out_rows.h"
#include "../../include/tetra_rx_out.h"
#include "compact_core.hpp"
#include "rx_handle.hpp"
#include "rx_out_core.hpp"

namespace {

constexpr int kTile = 128;            // rows per workgroup of k_out_count / k_out_write
constexpr int kMaxRowBytes = 268;     // SCH/F byte per bit

struct OutKind {                      // one selected kind of one parity
    const uint8_t* t2;                // [rows][out_stride] type-2 rows (type-1 bits first)
    const int32_t* ok;                // [rows]
    const tetra_rx_block_t* blocks;   // [rows]
    const int32_t* n_rows;            // [1] rows the call decoded
    int kind, out_stride, nb, rb;
};
struct OutArgs {
    OutKind k[TETRA_RX_N_KINDS];
    int nsel, flags, tiles, max_rows;
};
struct Layout {                       // what k_out_layout leaves for k_out_write
    int status;
    int n_dec[TETRA_RX_N_KINDS];
    uint64_t blocks_off[TETRA_RX_N_KINDS], bits_off[TETRA_RX_N_KINDS];
};

__device__ __forceinline__ int rows_of(const OutKind& k, int max_rows) {
    const int n = *k.n_rows;
    return n < 0 ? 0 : (n > max_rows ? max_rows : n);
}

// kept rows per tile (CRC-good only)
__global__ __launch_bounds__(kTile) void k_out_count(const OutArgs a, int32_t* __restrict__ tile_cnt) {
    const OutKind& k = a.k[blockIdx.y];
    const int n = rows_of(k, a.max_rows);
    const int t0 = (int)blockIdx.x * kTile;
    if (t0 >= n) return;
    const int i = t0 + (int)threadIdx.x;
    compact_core::block_count<1>(i < n && k.ok[i] != 0, tile_cnt + blockIdx.y * a.tiles, a.tiles, blockIdx.x);
}

// one workgroup: tile counts -> tile offsets, layout, header
__global__ __launch_bounds__(compact_core::kScanThreads) void k_out_layout(const OutArgs a, int32_t* __restrict__ tile_off, Layout* __restrict__ lay,
                                                                           uint8_t* __restrict__ dst, uint64_t capacity, long long call) {
    __shared__ int kept[TETRA_RX_N_KINDS], dec[TETRA_RX_N_KINDS];
    __shared__ __attribute__((aligned(16))) tetra_rx_out_header_t hd;
    const int t = (int)threadIdx.x;
    int tiles[TETRA_RX_N_KINDS];                           // each kind's own tile count; a kind not selected has none
#pragma unroll
    for (int s = 0; s < TETRA_RX_N_KINDS; s++) {
        const int n = s < a.nsel ? rows_of(a.k[s], a.max_rows) : 0;
        tiles[s] = (n + kTile - 1) / kTile;
        if (t == 0) kept[s] = dec[s] = n;
    }
    if (a.flags & TETRA_RX_OUT_CRC_GOOD) {
        __syncthreads();                                   // (kept[] is written twice)
        compact_core::scan_counts<TETRA_RX_N_KINDS>(tile_off, a.tiles, tiles, kept);
    }
    __syncthreads();
    if (t == 0) {
        int kinds[TETRA_RX_N_KINDS], nk[TETRA_RX_N_KINDS], nd[TETRA_RX_N_KINDS];
        for (int s = 0; s < a.nsel; s++) { kinds[s] = a.k[s].kind; nk[s] = kept[s]; nd[s] = dec[s]; }
        const uint64_t bytes = rx_out::layout(&hd, kinds, nk, nd, a.nsel, a.flags);
        hd.magic = TETRA_RX_OUT_MAGIC;
        hd.status = bytes <= capacity ? TETRA_OK : TETRA_ERR_SIZE;
        hd.flags = a.flags;
        hd.call = call;
        lay->status = hd.status;
        for (int s = 0; s < TETRA_RX_N_KINDS; s++) {
            lay->n_dec[s] = s < a.nsel ? dec[s] : 0;
            lay->blocks_off[s] = hd.kinds[s].blocks_offset;
            lay->bits_off[s] = hd.kinds[s].bits_offset;
        }
    }
    __syncthreads();
    constexpr int kWords = (int)(sizeof(tetra_rx_out_header_t) / 16);      // the enqueue checked capacity >= the header
    if (t < kWords) reinterpret_cast<uint4*>(dst)[t] = reinterpret_cast<const uint4*>(&hd)[t];
}

// the kept rows of one tile of one kind
__global__ __launch_bounds__(256) void k_out_write(const OutArgs a, const int32_t* __restrict__ tile_off, const Layout* __restrict__ lay,
                                                   uint8_t* __restrict__ dst) {
    __shared__ __attribute__((aligned(16))) uint8_t sbits[16 + kTile * kMaxRowBytes];
    __shared__ __attribute__((aligned(16))) uint64_t slab[2 + kTile * 3];
    __shared__ uint8_t src[kTile];
    if (lay->status != TETRA_OK) return;
    const int s = (int)blockIdx.y;
    const OutKind& k = a.k[s];
    const int n = lay->n_dec[s];
    const int t0 = (int)blockIdx.x * kTile;
    if (t0 >= n) return;
    const int t = (int)threadIdx.x;
    const bool crc = (a.flags & TETRA_RX_OUT_CRC_GOOD) != 0;
    const int base = crc ? tile_off[s * a.tiles + blockIdx.x] : t0;      // first output row of the tile
    // compaction of the tile's kept rows (waves 0 and 1 hold one row per lane)
    const bool keep = t < kTile && t0 + t < n && (!crc || k.ok[t0 + t] != 0);
    int at[1], cnt;
    compact_core::block_rank<1, kTile>(keep, at, &cnt);
    if (keep) src[at[0]] = (uint8_t)t;
    __syncthreads();
    if (cnt == 0) return;
    // labels: 3 words per row; slab[lshift + 3 r + j] holds output word (first word + 3 r + j), lshift = that word's parity, so
    // slab[2 c .. 2 c + 1] is the 16-byte aligned chunk c of the output
    const uint64_t lw0 = (lay->blocks_off[s] >> 3) + 3ull * (uint64_t)base;
    const int lshift = (int)(lw0 & 1);
    const uint64_t* blk = reinterpret_cast<const uint64_t*>(k.blocks);
    for (int i = t; i < 3 * cnt; i += 256) {
        const int r = i / 3, j = i - 3 * r;
        slab[lshift + i] = blk[(size_t)(t0 + src[r]) * 3 + j];
    }
    // type-1 rows, the same way at byte granularity: sbits[bshift + o] = output byte (first byte + o)
    const uint64_t b0 = lay->bits_off[s] + (uint64_t)k.rb * (uint64_t)base;
    const int bshift = (int)(b0 & 15);
    const int total = cnt * k.rb;
    if (a.flags & TETRA_RX_OUT_PACKED) {
        for (int o = t; o < total; o += 256) {
            const int r = o / k.rb, q = o - r * k.rb;
            const uint64_t v = *reinterpret_cast<const uint64_t*>(k.t2 + (size_t)(t0 + src[r]) * k.out_stride + 8 * q);
            sbits[bshift + o] = (uint8_t)rx_out::pack8(v, k.nb - 8 * q);
        }
    } else {          // two bytes per step: every kind's bit count and the shift are even
        const int half = k.rb >> 1;
        for (int o = t; o < total >> 1; o += 256) {
            const int r = o / half, q = o - r * half;
            *reinterpret_cast<uint16_t*>(sbits + bshift + 2 * o) =
                *reinterpret_cast<const uint16_t*>(k.t2 + (size_t)(t0 + src[r]) * k.out_stride + 2 * q);
        }
    }
    __syncthreads();
    // 16-byte stores of the whole chunks, narrower ones at the two ends of each run
    uint64_t* lout = reinterpret_cast<uint64_t*>(dst) + (lw0 - lshift);
    const int lend = lshift + 3 * cnt;
    for (int c = t; 2 * c < lend; c += 256) {
        if (2 * c >= lshift && 2 * c + 2 <= lend) {
            reinterpret_cast<uint4*>(lout)[c] = reinterpret_cast<const uint4*>(slab)[c];
        } else {
            for (int j = 2 * c; j < 2 * c + 2; j++)
                if (j >= lshift && j < lend) lout[j] = slab[j];
        }
    }
    uint8_t* bout = dst + (b0 - bshift);
    const int bend = bshift + total;
    for (int c = t; 16 * c < bend; c += 256) {
        if (16 * c >= bshift && 16 * c + 16 <= bend) {
            reinterpret_cast<uint4*>(bout)[c] = reinterpret_cast<const uint4*>(sbits)[c];
        } else {
            for (int j = 16 * c; j < 16 * c + 16; j++)
                if (j >= bshift && j < bend) bout[j] = sbits[j];
        }
    }
}

// ---- the extension block (include/ext/tetra_rx_out_ext.h): two more launches around k_out_write, which stays what it is ----
//
//   k_out_count (CRC-good only), k_out_layout        as ever
//   k_out_ext_layout  ONE workgroup behind k_out_layout: the kept rows per kind from the SAME scanned tile counts (a tile's first
//                     output row, plus the last tile's own kept rows), the extension's layout and header -> dst; if classic part plus
//                     extension do not fit, the status of the classic header in dst and of the Layout k_out_write reads becomes
//                     TETRA_ERR_SIZE and bytes the total, so that nothing but the classic header is written
//   k_out_write       as ever
//   k_out_ext_write   per kind and tile: the kept rows' columns, ranked like the rows, staged in LDS and stored as contiguous runs
//                     (rx_out::ext_stage / ext_store); one more row of workgroups copies the call's per-channel snapshot

struct ExtKind {                      // one selected kind's columns of one parity (the distance lies in its type-2 rows: kAachDistByte)
    const uint32_t* biterr;
    const int32_t* rank;
};
struct ExtArgs {
    ExtKind k[TETRA_RX_N_KINDS];
    const uint8_t* snap;              // the parity's snapshot (rx_out::snap_offset)
    int extras, n_channels;
};
struct ExtLayout {                    // what k_out_ext_layout leaves for k_out_ext_write
    int status;
    int n_dec[TETRA_RX_N_KINDS];
    uint64_t col[TETRA_RX_N_KINDS][rx_out::kRowCols];      // 0: the kind has no such column
    uint64_t tab[rx_out::kChanTables];                     // 0: no such table
};

__global__ __launch_bounds__(kTile) void k_out_ext_layout(const OutArgs a, const ExtArgs x, const int32_t* __restrict__ tile_off, Layout* __restrict__ lay,
                                                          ExtLayout* __restrict__ xl, uint8_t* __restrict__ dst, uint64_t capacity, long long call) {
    __shared__ int kept[TETRA_RX_N_KINDS];
    __shared__ tetra_rx_out_header_t hd;
    __shared__ __attribute__((aligned(16))) tetra_rx_out_ext_header_t ex;
    __shared__ int fits;
    const int t = (int)threadIdx.x;
    for (int s = 0; s < a.nsel; s++) {                     // (n is the same in every thread: the barriers are met by all)
        const int n = lay->n_dec[s];
        int k = n;
        if ((a.flags & TETRA_RX_OUT_CRC_GOOD) && n > 0) {
            const int last = (n - 1) / kTile, i = last * kTile + t;
            k = tile_off[s * a.tiles + last] + __syncthreads_count(i < n && a.k[s].ok[i] != 0);
        }
        if (t == 0) kept[s] = k;
    }
    __syncthreads();
    if (t == 0) {
        int kinds[TETRA_RX_N_KINDS], nk[TETRA_RX_N_KINDS], nd[TETRA_RX_N_KINDS];
        for (int s = 0; s < a.nsel; s++) { kinds[s] = a.k[s].kind; nk[s] = kept[s]; nd[s] = lay->n_dec[s]; }
        const uint64_t classic = rx_out::layout(&hd, kinds, nk, nd, a.nsel, a.flags);
        const uint64_t total = rx_out::layout_ext(&ex, kinds, nk, a.nsel, classic, x.extras, x.n_channels);
        ex.magic = TETRA_RX_OUT_EXT_MAGIC;
        ex.call = call;
        fits = total <= capacity;
        if (!fits) {
            lay->status = TETRA_ERR_SIZE;
            reinterpret_cast<tetra_rx_out_header_t*>(dst)->status = TETRA_ERR_SIZE;
            reinterpret_cast<tetra_rx_out_header_t*>(dst)->bytes = total;
        }
        xl->status = fits ? TETRA_OK : TETRA_ERR_SIZE;
        for (int s = 0; s < TETRA_RX_N_KINDS; s++) {
            xl->n_dec[s] = s < a.nsel ? nd[s] : 0;
            xl->col[s][0] = ex.kinds[s].biterr_offset;
            xl->col[s][1] = ex.kinds[s].rank_offset;
            xl->col[s][2] = ex.kinds[s].aach_dist_offset;
        }
        xl->tab[0] = ex.cell_offset;
        xl->tab[1] = ex.sync_state_offset;
        xl->tab[2] = ex.sync_misses_offset;
        xl->tab[3] = ex.link_offset;
    }
    __syncthreads();
    constexpr int kWords = (int)(rx_out::kExtHeaderBytes / 16);
    if (fits && t < kWords) reinterpret_cast<uint4*>(dst + rx_out::align16(hd.bytes))[t] = reinterpret_cast<const uint4*>(&ex)[t];
}

__global__ __launch_bounds__(kTile) void k_out_ext_write(const OutArgs a, const ExtArgs x, const int32_t* __restrict__ tile_off,
                                                         const ExtLayout* __restrict__ xl, uint8_t* __restrict__ dst) {
    __shared__ __attribute__((aligned(16))) uint8_t scol[rx_out::kRowCols][16 + kTile * 4];
    __shared__ uint8_t src[kTile];
    if (xl->status != TETRA_OK) return;
    const int t = (int)threadIdx.x;
    const int s = (int)blockIdx.y;
    if (s == a.nsel) {                // the per-channel tables, 16 bytes per thread
        for (int j = 0; j < rx_out::kChanTables; j++)
            if (xl->tab[j])
                rx_out::table_copy(dst + xl->tab[j], x.snap + rx_out::snap_offset(j, x.n_channels), (uint64_t)rx_out::chan_elem_bytes(j) * (uint64_t)x.n_channels,
                                   (uint64_t)blockIdx.x * kTile + (uint64_t)t, (uint64_t)gridDim.x * kTile);
        return;
    }
    const uint64_t* col = xl->col[s];
    if (!(col[0] | col[1] | col[2])) return;
    const OutKind& k = a.k[s];
    const int n = xl->n_dec[s];
    const int t0 = (int)blockIdx.x * kTile;
    if (t0 >= n) return;
    const bool crc = (a.flags & TETRA_RX_OUT_CRC_GOOD) != 0;
    const int base = crc ? tile_off[s * a.tiles + blockIdx.x] : t0;      // first output row of the tile, as in k_out_write
    const bool keep = t0 + t < n && (!crc || k.ok[t0 + t] != 0);
    int at[1], cnt;
    compact_core::block_rank<1, kTile>(keep, at, &cnt);
    if (keep) src[at[0]] = (uint8_t)t;
    __syncthreads();
    if (cnt == 0) return;
    const uint64_t b0 = col[0] + 4ull * (uint64_t)base, b1 = col[1] + 4ull * (uint64_t)base, b2 = col[2] + (uint64_t)base;
    if (col[0]) rx_out::ext_stage<4>(scol[0], b0, reinterpret_cast<const uint8_t*>(x.k[s].biterr), 4, t0, src, cnt, t, kTile);
    if (col[1]) rx_out::ext_stage<4>(scol[1], b1, reinterpret_cast<const uint8_t*>(x.k[s].rank), 4, t0, src, cnt, t, kTile);
    if (col[2]) rx_out::ext_stage<1>(scol[2], b2, k.t2 + kAachDistByte, (size_t)k.out_stride, t0, src, cnt, t, kTile);
    __syncthreads();
    if (col[0]) rx_out::ext_store<4>(dst, b0, scol[0], cnt, t, kTile);
    if (col[1]) rx_out::ext_store<4>(dst, b1, scol[1], cnt, t, kTile);
    if (col[2]) rx_out::ext_store<1>(dst, b2, scol[2], cnt, t, kTile);
}

// kinds (0 = every configured kind) -> the handle's selection; statuses as tetra_rx_out.h
int select_kinds(const tetra_rx* h, int kinds, int* sel) {
    if (kinds & ~((1 << TETRA_RX_N_KINDS) - 1)) return TETRA_ERR_ARG;
    if (kinds == 0) kinds = h->kinds;
    if (kinds & ~h->kinds) return TETRA_ERR_UNSUPPORTED;
    *sel = kinds;
    return TETRA_OK;
}

// The event to wait on for every delivery of `call` so far: the latest delivery of it in the ring; for a call older than every
// delivery in the ring, the oldest of them (the fetch stream runs deliveries in order, so it completes after any older one).
// -1: no delivery of that call was enqueued.
int ring_slot(const tetra_rx* h, int64_t call) {
    if (call < 0 || call >= h->calls) return -1;
    int hit = -1, oldest = -1;
    long long min_call = -1;
    for (int i = 0; i < tetra_rx::kOutRing; i++) {
        if (h->ring_call[i] < 0) continue;
        if (h->ring_call[i] == call && (hit < 0 || h->ring_seq[i] > h->ring_seq[hit])) hit = i;
        if (oldest < 0 || h->ring_seq[i] < h->ring_seq[oldest]) oldest = i;
        if (min_call < 0 || h->ring_call[i] < min_call) min_call = h->ring_call[i];
    }
    if (hit >= 0) return hit;
    return oldest >= 0 && call < min_call ? oldest : -1;
}

// TETRA_ERR_UNSUPPORTED for an extra whose flag the handle was created without, as its blocking fetch answers
int extras_supported(const tetra_rx* h, int extras) {
    for (int c = 0; c < rx_out::kRowCols; c++)
        if (extras & rx_out::row_extra(c)) TETRA_TRY(row_col::status(h, c));
    for (int t = 0; t < rx_out::kChanTables; t++)
        if (extras & rx_out::chan_extra(t)) TETRA_TRY(chan_tab::status(h, t));
    return TETRA_OK;
}

// where the kernels write: device memory on GPU `device`, or page-locked host memory through its device address; 16-byte aligned
int resolve_dst(void* dst, int device, uint8_t** out) {
    hipPointerAttribute_t at = {};
    if (hipPointerGetAttributes(&at, dst) != hipSuccess) {
        (void)hipGetLastError();
        return TETRA_ERR_ARG;
    }
    uint8_t* d = nullptr;
    if (at.type == hipMemoryTypeDevice) {
        if (at.device != device) return TETRA_ERR_ARG;
        d = static_cast<uint8_t*>(dst);
    } else if (at.type == hipMemoryTypeHost) {
        void* p = nullptr;
        if (hipHostGetDevicePointer(&p, dst, 0) != hipSuccess || !p) {
            (void)hipGetLastError();
            return TETRA_ERR_ARG;
        }
        d = static_cast<uint8_t*>(p);
    } else {
        return TETRA_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(d) & 15) return TETRA_ERR_ALIGN;
    *out = d;
    return TETRA_OK;
}

// The launches of one delivery on s, for the chain's rows (enqueue) and a caller's (tetra_rx_out_write_rows_device) alike.
// x.extras = 0: count (CRC-good only), layout, write, and nothing else; xl is not looked at then.
// tile_off [TETRA_RX_N_KINDS][a.tiles]: k_out_count's counts, scanned in place by k_out_layout
void launch(const OutArgs& a, const ExtArgs& x, uint8_t* d, uint64_t capacity, long long c, int32_t* tile_off, Layout* lay, ExtLayout* xl,
            hipStream_t s) {
    const unsigned tiles = (unsigned)a.tiles;
    if (a.flags & TETRA_RX_OUT_CRC_GOOD) hipLaunchKernelGGL(k_out_count, dim3(tiles, (unsigned)a.nsel), dim3(kTile), 0, s, a, tile_off);
    hipLaunchKernelGGL(k_out_layout, dim3(1), dim3(compact_core::kScanThreads), 0, s, a, tile_off, lay, d, capacity, c);
    if (x.extras) hipLaunchKernelGGL(k_out_ext_layout, dim3(1), dim3(kTile), 0, s, a, x, tile_off, lay, xl, d, capacity, c);
    hipLaunchKernelGGL(k_out_write, dim3(tiles, (unsigned)a.nsel), dim3(256), 0, s, a, tile_off, lay, d);
    if (x.extras) hipLaunchKernelGGL(k_out_ext_write, dim3(tiles, (unsigned)a.nsel + 1), dim3(kTile), 0, s, a, x, tile_off, xl, d);
}

// one selected kind of a launch
OutKind out_kind(int kind, const uint8_t* t2, int stride, const int32_t* ok, const tetra_rx_block_t* blocks, const int32_t* n_rows, int flags) {
    OutKind o = {};
    o.t2 = t2;
    o.ok = ok;
    o.blocks = blocks;
    o.n_rows = n_rows;
    o.kind = kind;
    o.out_stride = stride;
    o.nb = kKinds[kind].type1_bits;
    o.rb = rx_out::row_bytes(kind, flags);
    return o;
}

// the caller's workspace (tetra_rx_out_rows.h): the tile counts, the layout, the extension's layout, each on its own 16 bytes
struct RowsWork {
    size_t lay, xl, bytes;
    explicit RowsWork(int max_rows) {
        const size_t tiles = ((size_t)max_rows + kTile - 1) / kTile;
        lay = (size_t)rx_out::align16(sizeof(int32_t) * TETRA_RX_N_KINDS * tiles);
        xl = lay + (size_t)rx_out::align16(sizeof(Layout));
        bytes = xl + (size_t)rx_out::align16(sizeof(ExtLayout));
    }
};

int enqueue(tetra_rx* h, int which, int kinds, int flags, int extras, void* dst, uint64_t capacity, int64_t* call);

}  // namespace

extern "C" {

int tetra_rx_out_bound(tetra_rx_t* h, int kinds, int flags, uint64_t* bytes) {
    if (!h || !bytes || (flags & ~rx_out::kFlagsAll)) return TETRA_ERR_ARG;
    int sel = 0;
    TETRA_TRY(select_kinds(h, kinds, &sel));
    // every frame slot one burst type: its kinds and the AACH (which every burst carries) have a row per slot, the others none
    uint64_t worst = 0;
    for (int list : { TETRA_LIST_SYNC, TETRA_LIST_NORM_1, TETRA_LIST_NORM_2 }) {
        uint64_t b = 0;
        for (int k = 0; k < TETRA_RX_N_KINDS; k++)
            if ((sel & (1 << k)) && (kKinds[k].list == list || kKinds[k].list == TETRA_LIST_ANY))
                b += (uint64_t)h->rows * (sizeof(tetra_rx_block_t) + (uint64_t)rx_out::row_bytes(k, flags));
        worst = b > worst ? b : worst;
    }
    *bytes = rx_out::kHeaderBytes + worst + rx_out::kPadPerKind * (uint64_t)__builtin_popcount((unsigned)sel);
    return TETRA_OK;
}

int tetra_rx_out_bound_ext(tetra_rx_t* h, int kinds, int flags, int extras, uint64_t* bytes) {
    if (!h || !bytes || (flags & ~rx_out::kFlagsAll) || (extras & ~rx_out::kExtrasAll)) return TETRA_ERR_ARG;
    int sel = 0;
    TETRA_TRY(select_kinds(h, kinds, &sel));
    TETRA_TRY(extras_supported(h, extras));
    TETRA_TRY(tetra_rx_out_bound(h, kinds, flags, bytes));
    if (!extras) return TETRA_OK;
    // the same worst case: every frame slot one burst type; every section starts on its own 16 bytes
    uint64_t worst = 0, pads = 16 + 16 * (uint64_t)rx_out::kChanTables;
    for (int list : { TETRA_LIST_SYNC, TETRA_LIST_NORM_1, TETRA_LIST_NORM_2 }) {
        uint64_t b = 0;
        for (int k = 0; k < TETRA_RX_N_KINDS; k++)
            if ((sel & (1 << k)) && (kKinds[k].list == list || kKinds[k].list == TETRA_LIST_ANY))
                for (int c = 0; c < rx_out::kRowCols; c++)
                    if ((extras & rx_out::row_extra(c)) && row_col::status(h, c, k) == TETRA_OK) b += (uint64_t)h->rows * (uint64_t)rx_out::row_elem_bytes(c);
        worst = b > worst ? b : worst;
    }
    for (int t = 0; t < rx_out::kChanTables; t++)
        if (extras & rx_out::chan_extra(t)) worst += (uint64_t)rx_out::chan_elem_bytes(t) * (uint64_t)h->C;
    pads += 16 * (uint64_t)rx_out::kRowCols * (uint64_t)__builtin_popcount((unsigned)sel);
    *bytes += rx_out::kExtHeaderBytes + worst + pads;
    return TETRA_OK;
}

int tetra_rx_out_set_snapshot(tetra_rx_t* h, int chan_extras) {
    if (!h || (chan_extras & ~rx_out::kExtrasChan)) return TETRA_ERR_ARG;
    TETRA_TRY(extras_supported(h, chan_extras));
    if (chan_extras) {
        DeviceGuard g(h->device);
        if (!g.ok) return TETRA_ERR_NO_DEVICE;
        for (auto& s : h->snap)
            if (s.reserve((size_t)rx_out::snap_bytes(h->C)) != hipSuccess) {
                (void)hipGetLastError();
                return TETRA_ERR_NOMEM;
            }
    }
    h->snap_mask = chan_extras;
    return TETRA_OK;
}

int tetra_rx_out_enqueue(tetra_rx_t* h, int which, int kinds, int flags, void* dst, uint64_t capacity, int64_t* call) {
    return enqueue(h, which, kinds, flags, 0, dst, capacity, call);
}

int tetra_rx_out_enqueue_ext(tetra_rx_t* h, int which, int kinds, int flags, int extras, void* dst, uint64_t capacity, int64_t* call) {
    if (extras & ~rx_out::kExtrasAll) return TETRA_ERR_ARG;
    return enqueue(h, which, kinds, flags, extras, dst, capacity, call);
}

int tetra_rx_out_view_ext(const void* buf, uint64_t bytes, int kind, const uint32_t** biterr, const int32_t** rank, const uint8_t** aach_dist,
                          int* n_rows) {
    return rx_out::view_ext(buf, bytes, kind, biterr, rank, aach_dist, n_rows);
}

int tetra_rx_out_view_channels(const void* buf, uint64_t bytes, const tetra_lmac_cell_state_t** cell, const tetra_bsync_state_t** sync,
                               const int32_t** misses, const tetra_rx_link_t** link, int* n_channels) {
    return rx_out::view_channels(buf, bytes, cell, sync, misses, link, n_channels);
}

}  // extern "C"

namespace {

// tetra_rx_out_enqueue (extras = 0: its launches and nothing else) and tetra_rx_out_enqueue_ext
int enqueue(tetra_rx* h, int which, int kinds, int flags, int extras, void* dst, uint64_t capacity, int64_t* call) {
    if (!h || !dst || which < 0 || which > 1 || (flags & ~rx_out::kFlagsAll)) return TETRA_ERR_ARG;
    int sel = 0;
    TETRA_TRY(select_kinds(h, kinds, &sel));
    TETRA_TRY(extras_supported(h, extras));
    if (h->calls <= which) return TETRA_ERR_ARG;
    const int b = (int)((h->calls - 1 - which) & 1);
    if (extras & rx_out::kExtrasChan & ~h->snap_taken[b]) return TETRA_ERR_ARG;      // that call's tail took no such snapshot
    if (capacity < rx_out::kHeaderBytes) return TETRA_ERR_SIZE;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    uint8_t* d = nullptr;
    TETRA_TRY(resolve_dst(dst, h->device, &d));
    const int tiles = (h->rows + kTile - 1) / kTile;
    if (h->out_tiles.reserve(sizeof(int32_t) * TETRA_RX_N_KINDS * (size_t)tiles) != hipSuccess ||
        h->out_layout.reserve(sizeof(Layout)) != hipSuccess) {
        (void)hipGetLastError();
        return TETRA_ERR_NOMEM;
    }
    OutArgs a = {};
    for (int k = 0; k < TETRA_RX_N_KINDS; k++) {
        if (!(sel & (1 << k))) continue;
        const KindBufs& r = h->res[b][k];
        a.k[a.nsel++] = out_kind(k, r.t2, kKinds[k].out_stride, r.ok, r.blocks, r.n_rows, flags);
    }
    a.flags = flags;
    a.tiles = tiles;
    a.max_rows = h->rows;
    ExtArgs x = {};
    ExtLayout* xl = nullptr;
    if (extras) {
        if (h->out_ext_layout.reserve(sizeof(ExtLayout)) != hipSuccess) {
            (void)hipGetLastError();
            return TETRA_ERR_NOMEM;
        }
        xl = reinterpret_cast<ExtLayout*>(h->out_ext_layout.get());
        for (int i = 0; i < a.nsel; i++) {
            x.k[i].biterr = reinterpret_cast<const uint32_t*>(row_col::src(h, b, a.k[i].kind, COL_BITERR).base);
            x.k[i].rank = reinterpret_cast<const int32_t*>(row_col::src(h, b, a.k[i].kind, COL_RANK).base);
        }
        x.snap = h->snap[b];
        x.extras = extras;
        x.n_channels = h->C;
    }
    int32_t* tile_off = h->out_tiles;
    for (auto& e : h->ring_ev)
        if (!e) HIP_TRY(h, hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
    Layout* lay = reinterpret_cast<Layout*>(h->out_layout.get());
    const long long c = h->calls - 1 - which;
    hipStream_t s = h->fetch_s;
    HIP_TRY(h, hipStreamWaitEvent(s, h->ev_tail[b], 0));
    launch(a, x, d, capacity, c, tile_off, lay, xl, s);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(h->ev_out[b], s));
    h->out_pending[b] = true;
    const int slot = (int)(h->out_seq % tetra_rx::kOutRing);
    HIP_TRY(h, hipEventRecord(h->ring_ev[slot], s));
    h->ring_call[slot] = c;
    h->ring_seq[slot] = h->out_seq++;
    if (call) *call = c;
    return TETRA_OK;
}

}  // namespace

extern "C" {

size_t tetra_rx_out_rows_workspace_bytes(int max_rows) { return max_rows < 1 ? 0 : RowsWork(max_rows).bytes; }

int tetra_rx_out_write_rows_device(const tetra_rx_out_rows_t* kinds, int n_kinds, int max_rows, int flags, int row_extras, int64_t call, void* dst,
                                   uint64_t capacity, void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    if (!kinds || !dst || !d_workspace || n_kinds < 1 || n_kinds > TETRA_RX_N_KINDS || max_rows < 1 || (flags & ~rx_out::kFlagsAll) ||
        (row_extras & ~rx_out::kExtrasRow))
        return TETRA_ERR_ARG;
    const auto off_grid = [](const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; };
    OutArgs a = {};
    ExtArgs x = {};
    bool misaligned = off_grid(d_workspace, 16);
    for (int i = 0; i < n_kinds; i++) {
        const tetra_rx_out_rows_t& r = kinds[i];
        if (r.kind < 0 || r.kind >= TETRA_RX_N_KINDS || (i > 0 && r.kind <= kinds[i - 1].kind)) return TETRA_ERR_ARG;
        if (!r.d_type2 || !r.d_crc_ok || !r.d_blocks || !r.d_n_rows) return TETRA_ERR_ARG;
        if (r.type2_stride < 8 * ((kKinds[r.kind].type1_bits + 7) / 8)) return TETRA_ERR_ARG;
        const bool coded = rx_out::kind_has(r.kind, COL_BITERR);
        if (coded && (((row_extras & TETRA_RX_OUT_EXT_ROW_BITERR) && !r.d_biterr) || ((row_extras & TETRA_RX_OUT_EXT_ROW_LIST_RANK) && !r.d_rank)))
            return TETRA_ERR_ARG;
        misaligned = misaligned || (r.type2_stride & 7) || off_grid(r.d_type2, 8) || off_grid(r.d_blocks, 8) || off_grid(r.d_crc_ok, 4) ||
                     off_grid(r.d_n_rows, 4) || off_grid(r.d_biterr, 4) || off_grid(r.d_rank, 4);
        a.k[a.nsel++] = out_kind(r.kind, r.d_type2, r.type2_stride, r.d_crc_ok, r.d_blocks, r.d_n_rows, flags);
        x.k[i].biterr = r.d_biterr;
        x.k[i].rank = r.d_rank;
    }
    const RowsWork w(max_rows);
    if (capacity < rx_out::kHeaderBytes || workspace_bytes < w.bytes) return TETRA_ERR_SIZE;
    int device = -1;
    if (hipGetDevice(&device) != hipSuccess) {
        (void)hipGetLastError();
        return TETRA_ERR_NO_DEVICE;
    }
    uint8_t* d = nullptr;
    const int rc = resolve_dst(dst, device, &d);
    if (rc != TETRA_OK && rc != TETRA_ERR_ALIGN) return rc;
    if (misaligned || rc == TETRA_ERR_ALIGN) return TETRA_ERR_ALIGN;
    a.flags = flags;
    a.tiles = (int)(((size_t)max_rows + kTile - 1) / kTile);
    a.max_rows = max_rows;
    x.extras = row_extras;      // (no snapshot, no channels: the tables are a handle's)
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    launch(a, x, d, capacity, call, reinterpret_cast<int32_t*>(ws), reinterpret_cast<Layout*>(ws + w.lay), reinterpret_cast<ExtLayout*>(ws + w.xl),
           static_cast<hipStream_t>(hip_stream));
    return hipGetLastError() == hipSuccess ? TETRA_OK : TETRA_ERR_HIP;
}

int tetra_rx_out_query(tetra_rx_t* h, int64_t call) {
    if (!h) return TETRA_ERR_ARG;
    const int i = ring_slot(h, call);
    if (i < 0) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    const hipError_t e = hipEventQuery(h->ring_ev[i]);
    if (e == hipErrorNotReady) return 1;
    HIP_TRY(h, e);
    return TETRA_OK;
}

int tetra_rx_out_wait(tetra_rx_t* h, int64_t call) {
    if (!h) return TETRA_ERR_ARG;
    const int i = ring_slot(h, call);
    if (i < 0) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipEventSynchronize(h->ring_ev[i]));
    return TETRA_OK;
}

void* tetra_rx_out_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

void tetra_rx_out_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

int tetra_rx_out_view(const void* buf, uint64_t bytes, int kind, const tetra_rx_block_t** blocks, const uint8_t** bits, int* n_rows,
                      int* row_bytes) {
    return rx_out::view(buf, bytes, kind, blocks, bits, n_rows, row_bytes);
}

int tetra_rx_unpack_bits(const uint8_t* packed, int n_rows, int row_bytes, int n_bits, uint8_t* out, int out_stride) {
    return rx_out::unpack_bits(packed, n_rows, row_bytes, n_bits, out, out_stride);
}

}  // extern "C"

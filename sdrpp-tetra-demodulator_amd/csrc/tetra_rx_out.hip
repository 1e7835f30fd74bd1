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
// delivery that does not fit gets only its header.
#include <hip/hip_runtime.h>

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

int tetra_rx_out_enqueue(tetra_rx_t* h, int which, int kinds, int flags, void* dst, uint64_t capacity, int64_t* call) {
    if (!h || !dst || which < 0 || which > 1 || (flags & ~rx_out::kFlagsAll)) return TETRA_ERR_ARG;
    int sel = 0;
    TETRA_TRY(select_kinds(h, kinds, &sel));
    if (h->calls <= which) return TETRA_ERR_ARG;
    const int b = (int)((h->calls - 1 - which) & 1);
    if (capacity < rx_out::kHeaderBytes) return TETRA_ERR_SIZE;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    // where the kernels write: device memory on this GPU, or page-locked host memory through its device address
    hipPointerAttribute_t at = {};
    if (hipPointerGetAttributes(&at, dst) != hipSuccess) {
        (void)hipGetLastError();
        return TETRA_ERR_ARG;
    }
    uint8_t* d = nullptr;
    if (at.type == hipMemoryTypeDevice) {
        if (at.device != h->device) return TETRA_ERR_ARG;
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
        OutKind& o = a.k[a.nsel++];
        o.t2 = r.t2;
        o.ok = r.ok;
        o.blocks = r.blocks;
        o.n_rows = r.n_rows;
        o.kind = k;
        o.out_stride = kKinds[k].out_stride;
        o.nb = kKinds[k].type1_bits;
        o.rb = rx_out::row_bytes(k, flags);
    }
    a.flags = flags;
    a.tiles = tiles;
    a.max_rows = h->rows;
    int32_t* tile_off = h->out_tiles;                      // [kind][tile]: k_out_count's counts, scanned in place by k_out_layout
    for (auto& e : h->ring_ev)
        if (!e) HIP_TRY(h, hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
    Layout* lay = reinterpret_cast<Layout*>(h->out_layout.get());
    const long long c = h->calls - 1 - which;
    hipStream_t s = h->fetch_s;
    HIP_TRY(h, hipStreamWaitEvent(s, h->ev_tail[b], 0));
    if (flags & TETRA_RX_OUT_CRC_GOOD) hipLaunchKernelGGL(k_out_count, dim3((unsigned)tiles, (unsigned)a.nsel), dim3(kTile), 0, s, a, tile_off);
    hipLaunchKernelGGL(k_out_layout, dim3(1), dim3(compact_core::kScanThreads), 0, s, a, tile_off, lay, d, capacity, c);
    hipLaunchKernelGGL(k_out_write, dim3((unsigned)tiles, (unsigned)a.nsel), dim3(256), 0, s, a, tile_off, lay, d);
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

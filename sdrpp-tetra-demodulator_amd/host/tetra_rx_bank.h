// tetra_rx_bank.h -- C++ face of the receive chain behind one handle (include/tetra_rx.h), beside PI4DQPSKBank (pi4dqpsk_gpu.h):
// where PI4DQPSKBank stops at bits, TetraRxBank delivers what the reference's decoder block delivers to its upper MAC --
// tetra_burst_sync_in -> tetra_burst_rx_cb -> tp_sap_udata_ind (src/decoder/src/phy/tetra_burst_sync.c:54-155,
// phy/tetra_burst.c:343-393, lower_mac/tetra_lower_mac.c:148-275) -- for C channels on one GPU: decoded type-1 blocks with CRC
// verdict, TDMA time and channel, plus the per-channel cell state (tcd / t_phy_state).  Header-only; links libtetra_demod_hip.so.
#pragma once

#include <algorithm>
#include <cstdint>
#include <memory>
#include <vector>

#include "ext/tetra_aach_soft.h"
#include "ext/tetra_biterr.h"
#include "ext/tetra_gap.h"
#include "ext/tetra_handover.h"
#include "ext/tetra_list.h"
#include "ext/tetra_rx_out_ext.h"
#include "ext/tetra_sync_tol.h"
#include "ext/tetra_traffic.h"
#include "tetra_rx.h"
#include "tetra_rx_out.h"

namespace dsp {
namespace demod {

class TetraRxBank {
public:
    struct Blocks {                       // one kind's hand-overs of one call, in (channel, frame) order
        std::vector<tetra_rx_block_t> info;
        std::vector<uint8_t> type1;       // [info.size()][bitsPerBlock], one bit per byte
        int bitsPerBlock = 0;
        const uint8_t* bits(size_t row) const { return type1.data() + row * (size_t)bitsPerBlock; }
        // the opt-in columns of an extended delivery (ext/tetra_rx_out_ext.h), row for row beside info; empty where not delivered
        std::vector<uint32_t> biterr;     // errors | compared << 16 (coded kinds)
        std::vector<int32_t> rank;        // list-decoding rank (coded kinds)
        std::vector<uint8_t> aachDist;    // Reed-Muller distance (BBK)
        void clear() { info.clear(); type1.clear(); biterr.clear(); rank.clear(); aachDist.clear(); }
        // o's rows and columns behind these, its channels numbered from channelOffset on (a shard's share of a bank's)
        void append(const Blocks& o, int channelOffset) {
            bitsPerBlock = o.bitsPerBlock;
            const size_t at = info.size();
            info.insert(info.end(), o.info.begin(), o.info.end());
            for (size_t i = at; i < info.size(); i++) info[i].channel += channelOffset;
            type1.insert(type1.end(), o.type1.begin(), o.type1.end());
            biterr.insert(biterr.end(), o.biterr.begin(), o.biterr.end());
            rank.insert(rank.end(), o.rank.begin(), o.rank.end());
            aachDist.insert(aachDist.end(), o.aachDist.begin(), o.aachDist.end());
        }
    };
    struct Channels {                     // the per-channel state of the delivered call; empty where not delivered
        std::vector<tetra_lmac_cell_state_t> cell;
        std::vector<tetra_bsync_state_t> sync;
        std::vector<int32_t> misses;
        std::vector<tetra_rx_link_t> link;
        void clear() { cell.clear(); sync.clear(); misses.clear(); link.clear(); }
        // o's channels behind these (tables carry no channel numbers: the offset is their position)
        void append(const Channels& o, int /*channelOffset*/) {
            cell.insert(cell.end(), o.cell.begin(), o.cell.end());
            sync.insert(sync.end(), o.sync.begin(), o.sync.end());
            misses.insert(misses.end(), o.misses.begin(), o.misses.end());
            link.insert(link.end(), o.link.begin(), o.link.end());
        }
    };

    TetraRxBank() {}
    ~TetraRxBank() {
        if (h_) tetra_rx_destroy(h_);          // synchronises the device: no delivery still writes into out_
        for (auto& o : out_) tetra_rx_out_host_free(o.buf);
    }
    TetraRxBank(const TetraRxBank&) = delete;
    TetraRxBank& operator=(const TetraRxBank&) = delete;

    // cfg: tetra_rx_default_config() + demod.n_channels / max_samples / layout / device (+ kinds, flags).  Returns a TETRA_* status.
    int init(const tetra_rx_config_t& cfg) {
        if (h_) { tetra_rx_destroy(h_); h_ = nullptr; }
        for (auto& o : out_) { tetra_rx_out_host_free(o.buf); o = OutBuf(); }
        next_ = 0;
        channels_ = cfg.demod.n_channels;
        return tetra_rx_create(&cfg, &h_);
    }
    // in: n_channels x count complex samples (host) in cfg.demod.layout.  Enqueues the whole chain for this block and returns; the
    // blocks of the call BEFORE it are then complete or about to be (fetch(.., 1) waits for exactly that call's tail).
    int process(int count, const float* iq) { return tetra_rx_process(h_, iq, count); }
    // the same with the samples already on the GPU (what a channeliser leaves there), enqueued on the caller's stream
    int processDevice(int count, const float* dIq, void* hipStream) { return tetra_rx_process_device(h_, dIq, count, hipStream); }
    int wait() { return tetra_rx_wait(h_); }
    int reset() {
        out_[0].call = out_[1].call = -1;
        return tetra_rx_reset(h_);
    }
    // Decoded blocks of one kind (TETRA_RX_KIND_*) of the latest call (which = 0) or the one before it (1).
    int fetch(int kind, Blocks& out, int which = 0) {
        const int nb = tetra_rx_type1_bits(kind);
        if (nb < 0) return nb;
        int n = 0;
        int rc = tetra_rx_fetch(h_, which, kind, nullptr, nullptr, 0, 0, &n);
        if (rc != TETRA_OK) return rc;
        out.bitsPerBlock = nb;
        out.info.resize((size_t)n);
        out.type1.resize((size_t)n * (size_t)nb);
        if (n == 0) return TETRA_OK;
        return tetra_rx_fetch(h_, which, kind, out.info.data(), out.type1.data(), nb, n, &n);
    }
    // One-step hand-off (include/tetra_rx_out.h): every kind of `kinds` (0 = every configured kind) of the latest (which = 0) or
    // previous (1) call, gathered by the GPU into one of this bank's two page-locked buffers without waiting; *call names the delivered
    // call for collect(), which must come before the second deliver() after this one.  flags: TETRA_RX_OUT_*.
    // extras: TETRA_RX_OUT_EXT_* (ext/tetra_rx_out_ext.h) -- the rows' opt-in columns and, for the channel extras armed with
    // setSnapshot() when that call was processed, the call's per-channel state, in the same step.
    int deliver(int64_t* call, int which = 0, int kinds = 0, int flags = 0, int extras = 0) {
        if (!h_ || !call) return TETRA_ERR_ARG;
        // two buffers, taken in turn, each sized once for the largest delivery the handle can make (every kind, byte per bit); the
        // delivery stream runs them in order, so a buffer is only rewritten after the delivery before it has completed
        OutBuf& o = out_[next_];
        uint64_t need = o.bytes;
        if (extras) {                     // (also checks the extras against the handle's flags)
            const int rc = tetra_rx_out_bound_ext(h_, 0, 0, extras, &need);
            if (rc != TETRA_OK) return rc;
        }
        if (!o.buf || need > o.bytes) {
            if (!o.buf && !extras) {
                const int rc = tetra_rx_out_bound(h_, 0, 0, &need);
                if (rc != TETRA_OK) return rc;
            }
            if (o.buf) {                  // a larger one: the delivery last enqueued into this one has to be over first
                if (o.call >= 0) (void)tetra_rx_out_wait(h_, o.call);
                tetra_rx_out_host_free(o.buf);
                o = OutBuf();
            }
            if (!(o.buf = tetra_rx_out_host_alloc((size_t)need))) return TETRA_ERR_NOMEM;
            o.bytes = need;
        }
        const int rc = extras ? tetra_rx_out_enqueue_ext(h_, which, kinds, flags, extras, o.buf, o.bytes, call)
                              : tetra_rx_out_enqueue(h_, which, kinds, flags, o.buf, o.bytes, call);
        if (rc != TETRA_OK) return rc;
        o.call = *call;
        o.extras = extras;
        next_ ^= 1;
        return TETRA_OK;
    }
    // Waits for the delivery of `call` and copies its blocks out: out[kind] for every kind it holds (type-1 rows one bit per byte,
    // unpacked if the delivery was packed); the other entries are left empty.  For a delivery with extras the columns it holds come
    // with the rows, and *chans (may be null) receives its per-channel tables.
    int collect(int64_t call, Blocks out[TETRA_RX_N_KINDS], Channels* chans = nullptr) {
        if (!h_ || call < 0) return TETRA_ERR_ARG;
        int rc = tetra_rx_out_wait(h_, call);
        if (rc != TETRA_OK) return rc;
        const OutBuf* ob = out_[0].call == call ? &out_[0] : out_[1].call == call ? &out_[1] : nullptr;
        if (!ob) return TETRA_ERR_ARG;
        const OutBuf& o = *ob;
        for (int k = 0; k < TETRA_RX_N_KINDS; k++) {
            Blocks& b = out[k];
            b.clear();
            b.bitsPerBlock = tetra_rx_type1_bits(k);
            const tetra_rx_block_t* blk = nullptr;
            const uint8_t* bits = nullptr;
            int n = 0, rb = 0;
            rc = tetra_rx_out_view(o.buf, o.bytes, k, &blk, &bits, &n, &rb);
            if (rc == TETRA_ERR_UNSUPPORTED) continue;             // a kind the delivery does not hold
            if (rc != TETRA_OK) return rc;
            b.info.assign(blk, blk + n);
            if (o.extras) {
                const uint32_t* be = nullptr;
                const int32_t* rk = nullptr;
                const uint8_t* ad = nullptr;
                rc = tetra_rx_out_view_ext(o.buf, o.bytes, k, &be, &rk, &ad, nullptr);
                if (rc != TETRA_OK) return rc;
                if (be) b.biterr.assign(be, be + n);
                if (rk) b.rank.assign(rk, rk + n);
                if (ad) b.aachDist.assign(ad, ad + n);
            }
            if (rb == b.bitsPerBlock) {
                b.type1.assign(bits, bits + (size_t)n * (size_t)rb);
                continue;
            }
            b.type1.resize((size_t)n * (size_t)b.bitsPerBlock);
            rc = tetra_rx_unpack_bits(bits, n, rb, b.bitsPerBlock, b.type1.data(), b.bitsPerBlock);
            if (rc != TETRA_OK) return rc;
        }
        if (chans) {
            chans->clear();
            if (o.extras) {
                const tetra_lmac_cell_state_t* cell = nullptr;
                const tetra_bsync_state_t* sync = nullptr;
                const int32_t* misses = nullptr;
                const tetra_rx_link_t* link = nullptr;
                int n = 0;
                rc = tetra_rx_out_view_channels(o.buf, o.bytes, &cell, &sync, &misses, &link, &n);
                if (rc != TETRA_OK) return rc;
                if (cell) chans->cell.assign(cell, cell + n);
                if (sync) chans->sync.assign(sync, sync + n);
                if (misses) chans->misses.assign(misses, misses + n);
                if (link) chans->link.assign(link, link + n);
            }
        }
        return TETRA_OK;
    }
    // ext/tetra_rx_out_ext.h: the channel extras (TETRA_RX_OUT_EXT_CHAN_*) every tail from the next call on snapshots for deliver()
    int setSnapshot(int chanExtras) { return tetra_rx_out_set_snapshot(h_, chanExtras); }
    // tcd / t_phy_state of every channel (tetra_lower_mac.c:116, tetra_burst_sync.c:34 -- one per channel here)
    int cells(std::vector<tetra_lmac_cell_state_t>& out) { return table(tetra_rx_get_cell, out); }
    // TETRA_RX_FLAG_BITERR (tetra_biterr.h): errors | compared << 16 of a coded kind's rows, in fetch()'s order -- an estimate of the
    // channel's bit errors that is meaningful for rows with a good CRC ...
    int fetchBitErrors(int kind, std::vector<uint32_t>& out, int which = 0) { return column(tetra_rx_fetch_biterr, kind, out, which); }
    // ... and every channel's link figures since the last reset
    int links(std::vector<tetra_rx_link_t>& out) { return table(tetra_rx_get_link, out); }
    // TETRA_RX_FLAG_LIST (tetra_list.h): how many next-best paths (1..8) a CRC-failed block is decoded along from the next call on ...
    int setListCandidates(int maxCandidates) { return tetra_rx_set_list_candidates(h_, maxCandidates); }
    // ... and the rank of a coded kind's rows, in fetch()'s order: 0 = the decoder's own path passed, k >= 1 = rescued by candidate k,
    // -1 = failed and not rescued
    int fetchListRank(int kind, std::vector<int32_t>& out, int which = 0) { return column(tetra_rx_fetch_list_rank, kind, out, which); }
    // TETRA_RX_FLAG_AACH_SOFT (ext/tetra_aach_soft.h): the margin (1..930) from which a maximum-likelihood AACH row is accepted, from the
    // next call on ...
    int setAachMinMargin(int minMargin) { return tetra_rx_set_aach_min_margin(h_, minMargin); }
    // ... and the margin of every BBK row (saturated at 255; 0 = a tie), in fetch()'s order
    int fetchAachMargin(std::vector<uint16_t>& out, int which = 0) {
        int n = 0;
        const int rc = tetra_rx_fetch_aach_margin(h_, which, nullptr, 0, &n);
        if (rc != TETRA_OK) return rc;
        out.resize((size_t)n);
        return n ? tetra_rx_fetch_aach_margin(h_, which, out.data(), n, &n) : TETRA_OK;
    }
    int syncStates(std::vector<tetra_bsync_state_t>& out) { return table(tetra_rx_get_sync_state, out); }
    // The synchroniser's tolerant lock (ext/tetra_sync_tol.h; TETRA_RX_FLAG_SYNC_TOLERANT creates the chain with {3, 5, 16}): tol = null
    // returns to the reference's rule.  Between process calls; waits for the tail in flight.
    int setSyncTolerance(const tetra_bsync_tolerance_t* tol) { return tetra_rx_set_sync_tolerance(h_, tol); }
    // every channel's count of consecutive LOCKED frames without a training sequence
    int syncMisses(std::vector<int32_t>& out) { return table(tetra_rx_get_sync_misses, out); }
    // Retune with a donor (ext/tetra_handover.h): the listed channels restart, and channels[i] inherits frame timing, cell and TDMA clock
    // from donors[i] (-1: a plain restart); p = null: the header's defaults.  Enqueued on hipStream, not waited for.
    int handOver(const std::vector<int32_t>& channels, const std::vector<int32_t>& donors, const tetra_handover_params_t* p = nullptr,
                 void* hipStream = nullptr) {
        if (channels.size() != donors.size()) return TETRA_ERR_ARG;
        return tetra_rx_handover_channels_device(h_, channels.data(), donors.data(), (int)channels.size(), p, hipStream);
    }
    // A stream gap (ext/tetra_gap.h): the listed channels restart as their own heirs after elapsedBits bits that never arrived -- a channel
    // that was locked keeps its scrambling code and its TDMA clock, advanced by the slots that passed; p = null: the header's defaults.
    // Enqueued on hipStream, not waited for.
    int resume(const std::vector<int32_t>& channels, int64_t elapsedBits, const tetra_handover_params_t* p = nullptr, void* hipStream = nullptr) {
        return tetra_rx_resume_channels_device(h_, channels.data(), (int)channels.size(), elapsedBits, p, hipStream);
    }
    // ... and every channel's hand-over status
    int handoverStatus(std::vector<tetra_handover_status_t>& out) { return table(tetra_rx_get_handover, out); }
    // Traffic slots (ext/tetra_traffic.h): once per bank, at most maxRows rows per TCH kind and call (0: the handle's most) ...
    int enableTraffic(int maxRows = 0) { return tetra_rx_traffic_enable(h_, maxRows > 0 ? maxRows : tetra_rx_max_rows(h_)); }
    // ... the table entries of channels first .. first + slots.size() / 4 - 1, four per channel (timeslots 1..4), from the next call on;
    // enqueued on hipStream, not waited for ...
    int setTraffic(int first, const std::vector<tetra_rx_traffic_slot_t>& slots, void* hipStream = nullptr) {
        if (slots.size() % 4) return TETRA_ERR_ARG;
        return tetra_rx_set_traffic(h_, first, (int)(slots.size() / 4), slots.data(), hipStream);
    }
    // ... and the rows of one TCH kind (TETRA_LMAC_T_TCH_*) of the latest call (which = 0) or the one before it (1): type1 holds the
    // kind's type-2 bits (432 / 292 / 148 per row, the type-1 bits first), biterr the count words where the handle counts (the coded
    // kinds under TETRA_RX_FLAG_BITERR); *dropped (may be null): the rows routed beyond maxRows
    int fetchTraffic(int tchKind, Blocks& out, int* dropped = nullptr, int which = 0) {
        int n = 0;
        int rc = tetra_rx_fetch_traffic(h_, which, tchKind, nullptr, nullptr, 0, 0, nullptr, &n, dropped);
        if (rc != TETRA_OK) return rc;
        out.clear();
        out.bitsPerBlock = tchKind == TETRA_LMAC_T_TCH_7_2 ? 432 : tchKind == TETRA_LMAC_T_TCH_4_8 ? 292 : 148;
        out.info.resize((size_t)n);
        out.type1.resize((size_t)n * (size_t)out.bitsPerBlock);
        if (n == 0) return TETRA_OK;
        out.biterr.resize((size_t)n);
        rc = tetra_rx_fetch_traffic(h_, which, tchKind, out.info.data(), out.type1.data(), out.bitsPerBlock, n, out.biterr.data(), &n, dropped);
        if (rc != TETRA_ERR_UNSUPPORTED) return rc;
        out.biterr.clear();                  // no counts on this handle or for this kind
        return tetra_rx_fetch_traffic(h_, which, tchKind, out.info.data(), out.type1.data(), out.bitsPerBlock, n, nullptr, &n, dropped);
    }
    // the PI4DQPSK setters of the demodulators inside (tetra_demod_set_param ids); waits for work in flight first
    int setParam(int paramId, double value) {
        const int rc = tetra_rx_wait(h_);
        if (rc != TETRA_OK && rc != TETRA_ERR_OVERRUN) return rc;
        return tetra_demod_set_param(tetra_rx_demod(h_), paramId, value);
    }
    int channels() const { return channels_; }
    tetra_rx_t* handle() { return h_; }

private:
    // a row column's blocking fetch (fetch(h, which, kind, out, capacity, &n_rows)): asked for the row count, sized, asked for the rows
    template <class T, class Fetch> int column(Fetch fetch, int kind, std::vector<T>& out, int which) {
        int n = 0;
        const int rc = fetch(h_, which, kind, nullptr, 0, &n);
        if (rc != TETRA_OK) return rc;
        out.resize((size_t)n);
        return n ? fetch(h_, which, kind, out.data(), n, &n) : TETRA_OK;
    }
    // a per-channel getter (get(h, first, count, out)) for every channel
    template <class T, class Get> int table(Get get, std::vector<T>& out) {
        out.resize((size_t)channels_);
        return get(h_, 0, channels_, out.data());
    }
    struct OutBuf {
        void* buf = nullptr;
        uint64_t bytes = 0;
        int64_t call = -1;                // the call last delivered into it
        int extras = 0;                   // ... and the extras it was asked for
    };
    tetra_rx_t* h_ = nullptr;
    int channels_ = 0;
    OutBuf out_[2];
    int next_ = 0;
};

// The chain over several GPUs of a node, beside PI4DQPSKMultiBank: channels are independent receivers, so GPU g takes the channel
// range [g C / G, (g + 1) C / G) (the split of shard.py / bench.py --gpus N) and nothing crosses between the GPUs.  tetra_rx_process*
// only ENQUEUES (every handle has its own streams on its own device), so one host thread drives all shards; blocks come back with
// their channel numbers in the whole bank's numbering, shard after shard = (channel, frame) order.
class TetraRxMultiBank {
public:
    TetraRxMultiBank() {}
    TetraRxMultiBank(const TetraRxMultiBank&) = delete;
    TetraRxMultiBank& operator=(const TetraRxMultiBank&) = delete;

    // cfg.demod.n_channels = ALL channels (>= devices.size()); cfg.demod.device is ignored; one shard per entry of `devices` (an
    // ordinal may repeat: two shards on one GPU, e.g. for tests on a one-GPU box).
    int init(const tetra_rx_config_t& cfg, const std::vector<int>& devices) {
        shards_.clear();
        channels_ = cfg.demod.n_channels;
        const int G = (int)devices.size();
        if (G < 1 || channels_ < G) return TETRA_ERR_ARG;
        for (int g = 0; g < G; g++) {
            std::unique_ptr<Shard> s(new Shard());
            s->first = (int)((long long)g * channels_ / G);
            s->count = (int)((long long)(g + 1) * channels_ / G) - s->first;
            tetra_rx_config_t c = cfg;
            c.demod.n_channels = s->count;
            c.demod.device = devices[(size_t)g];
            const int rc = s->bank.init(c);
            if (rc != TETRA_OK) { shards_.clear(); return rc; }
            shards_.push_back(std::move(s));
        }
        return TETRA_OK;
    }
    // Samples already on the GPUs: dIq[s] = device pointer on shard s's device to its [count_s channels x count] samples (in
    // cfg.demod.layout), streams[s] = a HIP stream of that device (or null).  Enqueues on every shard and returns.
    int processDevice(int count, const float* const* dIq, void* const* streams) {
        for (size_t s = 0; s < shards_.size(); s++) {
            const int rc = shards_[s]->bank.processDevice(count, dIq[s], streams ? streams[s] : nullptr);
            if (rc != TETRA_OK) return rc;
        }
        return TETRA_OK;
    }
    // Host samples, channel major [n_channels][count] complex64: every shard copies its rows in and enqueues its chain.
    int process(int count, const float* iq) {
        return each([&](Shard& s) { return s.bank.process(count, iq + (size_t)2 * (size_t)s.first * (size_t)count); });
    }
    int wait() {
        int first = TETRA_OK;
        for (auto& s : shards_) { const int rc = s->bank.wait(); if (first == TETRA_OK) first = rc; }
        return first;
    }
    int reset() { return each([](Shard& s) { return s.bank.reset(); }); }
    int fetch(int kind, TetraRxBank::Blocks& out, int which = 0) {
        out.clear();
        TetraRxBank::Blocks part;
        return each([&](Shard& s) {
            const int rc = s.bank.fetch(kind, part, which);
            if (rc == TETRA_OK) out.append(part, s.first);
            return rc;
        });
    }
    // Every kind of `kinds` (0 = all configured) in one step per shard: every shard's delivery is enqueued first, then each is
    // collected, so the GPUs' transfers run side by side.  out[kind] as fetch() returns it (bank channel numbers, (channel, frame)
    // order, one bit per byte); kinds outside the delivery come back empty.
    // extras (ext/tetra_rx_out_ext.h): the shards' columns one after the other like their rows, and *chans (may be null) the per-channel
    // tables in the bank's channel order; the channel extras need setSnapshot() armed when that call was processed.
    int fetchAll(TetraRxBank::Blocks out[TETRA_RX_N_KINDS], int which = 0, int kinds = 0, int flags = 0, int extras = 0,
                 TetraRxBank::Channels* chans = nullptr) {
        for (int k = 0; k < TETRA_RX_N_KINDS; k++) { out[k].clear(); out[k].bitsPerBlock = tetra_rx_type1_bits(k); }
        if (chans) chans->clear();
        std::vector<int64_t> calls(shards_.size(), -1);
        for (size_t s = 0; s < shards_.size(); s++) {
            const int rc = shards_[s]->bank.deliver(&calls[s], which, kinds, flags, extras);
            if (rc != TETRA_OK) return rc;
        }
        TetraRxBank::Blocks part[TETRA_RX_N_KINDS];
        TetraRxBank::Channels cpart;
        for (size_t s = 0; s < shards_.size(); s++) {
            const int rc = shards_[s]->bank.collect(calls[s], part, chans ? &cpart : nullptr);
            if (rc != TETRA_OK) return rc;
            for (int k = 0; k < TETRA_RX_N_KINDS; k++) out[k].append(part[k], shards_[s]->first);
            if (chans) chans->append(cpart, shards_[s]->first);
        }
        return TETRA_OK;
    }
    int setSnapshot(int chanExtras) { return each([&](Shard& s) { return s.bank.setSnapshot(chanExtras); }); }
    int syncStates(std::vector<tetra_bsync_state_t>& out) { return gather(out, [](TetraRxBank& b, auto& part) { return b.syncStates(part); }); }
    int syncMisses(std::vector<int32_t>& out) { return gather(out, [](TetraRxBank& b, auto& part) { return b.syncMisses(part); }); }
    int cells(std::vector<tetra_lmac_cell_state_t>& out) { return gather(out, [](TetraRxBank& b, auto& part) { return b.cells(part); }); }
    // the shards' counts and link figures one after the other: fetch()'s row order, cells()'s channel order
    int fetchBitErrors(int kind, std::vector<uint32_t>& out, int which = 0) {
        return gather(out, [&](TetraRxBank& b, auto& part) { return b.fetchBitErrors(kind, part, which); });
    }
    int setListCandidates(int maxCandidates) { return each([&](Shard& s) { return s.bank.setListCandidates(maxCandidates); }); }
    int fetchListRank(int kind, std::vector<int32_t>& out, int which = 0) {
        return gather(out, [&](TetraRxBank& b, auto& part) { return b.fetchListRank(kind, part, which); });
    }
    int setAachMinMargin(int minMargin) { return each([&](Shard& s) { return s.bank.setAachMinMargin(minMargin); }); }
    int fetchAachMargin(std::vector<uint16_t>& out, int which = 0) {
        return gather(out, [&](TetraRxBank& b, auto& part) { return b.fetchAachMargin(part, which); });
    }
    int links(std::vector<tetra_rx_link_t>& out) { return gather(out, [](TetraRxBank& b, auto& part) { return b.links(part); }); }
    // Retune with a donor (ext/tetra_handover.h), in the bank's channel numbers: every shard is told its own entries.  Nothing crosses
    // between the GPUs, so a donor must lie in its heir's shard: TETRA_ERR_ARG otherwise (and for a channel outside the bank), nothing
    // enqueued on any shard.  streams[s]: a HIP stream of shard s's device (streams = null: the null streams).
    int handOver(const std::vector<int32_t>& channels, const std::vector<int32_t>& donors, const tetra_handover_params_t* p = nullptr,
                 void* const* streams = nullptr) {
        PerShard ch, dn;
        if (channels.size() != donors.size() || !split(channels, &donors, p, ch, dn)) return TETRA_ERR_ARG;
        for (size_t s = 0; s < shards_.size(); s++) {
            const int rc = shards_[s]->bank.handOver(ch[s], dn[s], p, streams ? streams[s] : nullptr);
            if (rc != TETRA_OK) return rc;
        }
        return TETRA_OK;
    }
    // A stream gap (ext/tetra_gap.h), in the bank's channel numbers: every shard is told its own entries.  Everything a shard would refuse
    // is refused here (TETRA_ERR_ARG), before the first shard is told anything.  streams as for handOver.
    int resume(const std::vector<int32_t>& channels, int64_t elapsedBits, const tetra_handover_params_t* p = nullptr, void* const* streams = nullptr) {
        PerShard ch, dn;
        if (elapsedBits < 0 || elapsedBits > TETRA_GAP_MAX_ELAPSED_BITS || !split(channels, nullptr, p, ch, dn)) return TETRA_ERR_ARG;
        for (size_t s = 0; s < shards_.size(); s++) {
            const int rc = shards_[s]->bank.resume(ch[s], elapsedBits, p, streams ? streams[s] : nullptr);
            if (rc != TETRA_OK) return rc;
        }
        return TETRA_OK;
    }
    int handoverStatus(std::vector<tetra_handover_status_t>& out) { return gather(out, [](TetraRxBank& b, auto& part) { return b.handoverStatus(part); }); }
    // Traffic slots (ext/tetra_traffic.h): every shard keeps up to maxRows rows per kind and call (0: its most) ...
    int enableTraffic(int maxRows = 0) { return each([&](Shard& s) { return s.bank.enableTraffic(maxRows); }); }
    // ... the table entries of the bank's channels first .. first + slots.size() / 4 - 1, every shard told its own; a range outside the
    // bank is TETRA_ERR_ARG with no shard told anything (an entry a shard refuses leaves the shards before it changed) ...
    int setTraffic(int first, const std::vector<tetra_rx_traffic_slot_t>& slots, void* const* streams = nullptr) {
        const long long count = (long long)(slots.size() / 4);
        if (slots.size() % 4 || first < 0 || first + count > channels_) return TETRA_ERR_ARG;
        for (size_t s = 0; s < shards_.size(); s++) {
            const long long lo = std::max<long long>(first, shards_[s]->first), hi = std::min<long long>(first + count, shards_[s]->first + shards_[s]->count);
            if (lo >= hi) continue;
            const std::vector<tetra_rx_traffic_slot_t> part(slots.begin() + (lo - first) * 4, slots.begin() + (hi - first) * 4);
            const int rc = shards_[s]->bank.setTraffic((int)(lo - shards_[s]->first), part, streams ? streams[s] : nullptr);
            if (rc != TETRA_OK) return rc;
        }
        return TETRA_OK;
    }
    // ... and the shards' rows one after the other: bank channel numbers, (channel, frame) order; *dropped: summed over the shards
    int fetchTraffic(int tchKind, TetraRxBank::Blocks& out, int* dropped = nullptr, int which = 0) {
        out.clear();
        if (dropped) *dropped = 0;
        TetraRxBank::Blocks part;
        return each([&](Shard& s) {
            int d = 0;
            const int rc = s.bank.fetchTraffic(tchKind, part, &d, which);
            if (rc == TETRA_OK) out.append(part, s.first);
            if (dropped) *dropped += d;
            return rc;
        });
    }
    int channels() const { return channels_; }
    int shards() const { return (int)shards_.size(); }
    void shardInfo(int shard, int& first, int& count) const { first = shards_[(size_t)shard]->first; count = shards_[(size_t)shard]->count; }
    TetraRxBank& shard(int s) { return shards_[(size_t)s]->bank; }

private:
    struct Shard {
        TetraRxBank bank;
        int first = 0, count = 0;
    };
    // the shard that holds channel c of the bank, or -1
    int shardOf(int c) const {
        for (size_t s = 0; s < shards_.size(); s++)
            if (c >= shards_[s]->first && c < shards_[s]->first + shards_[s]->count) return (int)s;
        return -1;
    }
    // the bounds of tetra_handover_params_t, which the public headers state in words only (csrc/bsync_core.hpp: kWindowMax, kAssistSlotsMax)
    enum { kWindowMax = 127, kMaxSlotsMax = 255 };
    typedef std::vector<std::vector<int32_t>> PerShard;
    // A restart's list in the bank's channel numbers, checked and split: ch[s] = shard s's entries in its own numbering, and with donors
    // (-1: none) dn[s] beside it.  false: something a shard would refuse -- a channel outside the bank or listed twice, a donor outside
    // its heir's shard or itself an heir, parameters out of range -- so that it is refused before any shard is told anything.
    bool split(const std::vector<int32_t>& channels, const std::vector<int32_t>* donors, const tetra_handover_params_t* p, PerShard& ch, PerShard& dn) const {
        if (p && (p->window < 0 || p->window > kWindowMax || p->max_slots < 1 || p->max_slots > kMaxSlotsMax)) return false;
        std::vector<char> listed((size_t)channels_, 0);
        for (int32_t c : channels) {
            if (c < 0 || c >= channels_ || listed[(size_t)c]) return false;
            listed[(size_t)c] = 1;
        }
        ch.assign(shards_.size(), {});
        dn.assign(shards_.size(), {});
        for (size_t i = 0; i < channels.size(); i++) {
            const int s = shardOf(channels[i]), first = shards_[(size_t)s]->first;
            ch[(size_t)s].push_back(channels[i] - first);
            if (!donors) continue;
            const int32_t d = (*donors)[i];
            if (d != -1 && (shardOf(d) != s || listed[(size_t)d])) return false;
            dn[(size_t)s].push_back(d == -1 ? -1 : d - first);
        }
        return true;
    }
    // tell every shard in turn: the first failure ends the round and is the result
    template <class Tell> int each(Tell tell) {
        for (auto& s : shards_) {
            const int rc = tell(*s);
            if (rc != TETRA_OK) return rc;
        }
        return TETRA_OK;
    }
    // ask every shard (ask(bank, part)) and put the answers one after the other: the shards' rows, or their channels, in the bank's order
    template <class T, class Ask> int gather(std::vector<T>& out, Ask ask) {
        out.clear();
        std::vector<T> part;
        return each([&](Shard& s) {
            const int rc = ask(s.bank, part);
            if (rc == TETRA_OK) out.insert(out.end(), part.begin(), part.end());
            return rc;
        });
    }
    std::vector<std::unique_ptr<Shard>> shards_;
    int channels_ = 0;
};

}  // namespace demod
}  // namespace dsp

// dpq_flat_ivf_device.h -- the key sink the list scans over raw rows share (dpq_flat_ivf.hip: fp32 rows, dpq_flat_ivf_u8.hip:
// byte rows).  Per (query, probed list) pair of a stretch a buffer of cap = 2 P2 keys in LDS, P2 the
// power of two >= max(top_k, 256); a count and a threshold per pair.  A key below its pair's threshold is appended by an
// LDS atomic on the count; when a buffer could overflow on the next tile of kFlatIvfTileRows rows, the buffers of the
// stretch are sorted side by side (one bitonic network, the same barriers for all), cut to top_k, and the thresholds
// become the k-th keys.  Below it, fill_tile: the tile of a scan under an id filter.  Included by the
// scans' .hip files only; every function is called by all 256 threads of a workgroup with arguments that are the same in
// every thread.
#pragma once
#include "dpq_flat.h"
#include "dpq_flat_ivf.h"

namespace dpq {
namespace {

constexpr uint32_t kNoRow = 0xffffffffu;  // a slot of the row tile beyond the list's end

int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

int scan_cap(int top_k) { return 2 * pow2_at_least(std::max(top_k, 256)); }

// Sorts nb buffers of n keys each (n a power of two >= 2), `stride` keys apart, ascending: ivf_bitonic's network over
// every buffer at once.  Every thread of the workgroup calls it.  Ends behind a barrier.
__device__ __forceinline__ void sort_buffers(uint64_t* buf, int nb, int n, int stride, int tid) {
    const int half = n >> 1, hs = __ffs(half) - 1, total = nb * half;
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < total; t += 256) {
                const int u = t & (half - 1);
                uint64_t* b = buf + (size_t)(t >> hs) * stride;
                const int i = ((u & ~(j - 1)) << 1) | (u & (j - 1));
                const int l = i | j;
                const uint64_t x = b[i], y = b[l];
                const bool up = (i & k) == 0;
                if ((x > y) == up) {
                    b[i] = y;
                    b[l] = x;
                }
            }
            __syncthreads();
        }
}

// The buffers of the stretch's nqs pairs, each padded to the power of two >= the largest count mx, sorted.  Behind a
// barrier that closed the appends; ends behind a barrier.
__device__ __forceinline__ void sink_sort_to(uint64_t* buf, const uint32_t* s_cnt, int nqs, int cap, uint32_t mx, int tid) {
    int n = 2;
    while ((uint32_t)n < mx) n <<= 1;
    for (int p = 0; p < nqs; ++p)
        for (int i = (int)s_cnt[p] + tid; i < n; i += 256) buf[(size_t)p * cap + i] = kFlatNoKey;
    __syncthreads();
    sort_buffers(buf, nqs, n, cap, tid);
}

// ... with the largest count found here.
__device__ __forceinline__ void sink_sort(uint64_t* buf, const uint32_t* s_cnt, int nqs, int cap, int tid) {
    uint32_t mx = 0u;
    for (int p = 0; p < nqs; ++p) mx = max(mx, s_cnt[p]);
    sink_sort_to(buf, s_cnt, nqs, cap, mx, tid);
}

// Between two tiles, behind the barrier that closed the first one's appends: when a buffer has no room for the next
// tile, sort, keep top_k, lower the thresholds.  The caller's next barrier publishes the counts and thresholds.
__device__ __forceinline__ void sink_make_room(uint64_t* buf, uint32_t* s_cnt, uint64_t* s_thr, int nqs, int cap, int top_k,
                                               int tid) {
    uint32_t mx = 0u;
    for (int p = 0; p < nqs; ++p) mx = max(mx, s_cnt[p]);
    if (mx + kFlatIvfTileRows > (uint32_t)cap) {
        sink_sort_to(buf, s_cnt, nqs, cap, mx, tid);
        if (tid < nqs) {
            const uint32_t c = s_cnt[tid];
            if (c >= (uint32_t)top_k) s_thr[tid] = buf[(size_t)tid * cap + top_k - 1];  // ids are unique in a list: the
            s_cnt[tid] = min(c, (uint32_t)top_k);                                      // strict test loses nothing
        }
    }
}

// The answer of one pair: the first min(cnt, top_k) keys of its sorted buffer, padded with -1 / +inf.
__device__ __forceinline__ void sink_emit(const uint64_t* b, uint32_t cnt, int top_k, int32_t* out_i, float* out_d, int tid) {
    for (int r = tid; r < top_k; r += 256) {
        const uint64_t key = (uint32_t)r < cnt ? b[r] : kFlatNoKey;
        out_i[r] = key != kFlatNoKey ? (int32_t)(key & 0xffffffffu) : -1;
        out_d[r] = key != kFlatNoKey ? __uint_as_float((uint32_t)(key >> 32)) : INFINITY;
    }
}

// ---- the range sink --------------------------------------------------------------------------------------
// A scan kernel's last template argument says where its keys go: kSinkTopK, the buffers above; kSinkCount and kSinkEmit,
// the two passes of a range search (dpq_flat_ivf.h's FlatIvfRange), which keep NO key buffers in LDS.  Both take a pair's
// threshold from the caller, once per stretch, and never lower it.  Count: a lane counts its passing keys in registers
// over all tiles of the stretch; at the stretch's end one wavefront reduction and one LDS atomic per wavefront and query,
// and the sum goes out under the pair's value word.  Emit: range_begin drops the pairs without hits and compacts the
// rest in place, so everything behind it -- the staged queries, the active wavefronts, the MFMA's N side, the binary
// scan's 4 / 8 / 16-query form -- sees a shorter stretch; a passing key takes its slot from an LDS atomic on its pair's
// counter and goes to the pool with an ordinary store.
constexpr int kSinkTopK = 0, kSinkCount = 1, kSinkEmit = 2;

// The kernels' last argument: nothing for the top-k sink.
template <int SINK> struct SinkArgs { FlatIvfRange r; };
template <> struct SinkArgs<kSinkTopK> {};

// The pair-offset words of the range modes; the top-k kernels declare none.
struct RangeLds {
    int64_t off[kFlatIvfGroupMax];  // emit: where a surviving pair's region starts in the pool
    uint32_t nk;                    // emit: the stretch's surviving pairs
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// The start of a stretch -- pairs s .. s + nqs - 1 of the run, nqs <= 16 -- in a range mode; every thread calls it behind
// a barrier that published s_val / s_q.  Returns the queries the stretch goes on with, the same in every thread: all of
// them when counting (the counts and thresholds are in place behind the caller's next barrier); when emitting, the pairs
// that have hits and whose query is of the launch's sub-batch, moved to the front of s_val / s_q in order, their counters,
// thresholds and pool offsets set, behind a barrier.  One wavefront compacts: its reads of a slot come before its writes.
template <int SINK>
__device__ __forceinline__ int range_begin(const FlatIvfRange& R, uint32_t* s_val, uint32_t* s_q, uint32_t* s_cnt, uint64_t* s_thr,
                                           RangeLds& rl, int s, int nqs, int tid) {
    if constexpr (SINK == kSinkCount) {
        if (tid < nqs) {
            s_cnt[tid] = 0u;
            s_thr[tid] = R.thr[s_q[s + tid]];
        }
        return nqs;
    } else {
        if (tid < 64) {
            uint32_t val = 0u, q = 0u;
            bool keep = false;
            if (tid < nqs) {
                val = s_val[s + tid];
                q = s_q[s + tid];
                keep = (int)q >= R.qa && (int)q < R.qb && R.counts[val] > 0;
            }
            const uint64_t m = __ballot(keep);
            if (keep) {
                const int slot = __popcll(m & (((uint64_t)1 << tid) - 1));
                s_val[s + slot] = val;
                s_q[s + slot] = q;
                s_cnt[slot] = 0u;
                s_thr[slot] = R.thr[q];
                rl.off[slot] = R.offs[val] - R.pool_base;
            }
            if (tid == 0) rl.nk = (uint32_t)__popcll(m);
        }
        __syncthreads();
        const int nk = (int)rl.nk;
        __syncthreads();  // a stretch without pairs is left at once: the next one's count must not overtake this read
        return nk;
    }
}

// Emit: the key of surviving pair qs to its next slot.
__device__ __forceinline__ void range_put(const FlatIvfRange& R, const RangeLds& rl, uint32_t* s_cnt, int qs, uint64_t key) {
    const int64_t at = rl.off[qs] + (int64_t)atomicAdd(&s_cnt[qs], 1u);
    if (at >= 0 && at < R.pool_n) R.pool[at] = key;
}

// Count: the end of a stretch, behind the atomics that added the wavefronts' sums to s_cnt.  list_read: the stretch had rows.
__device__ __forceinline__ void range_counts_out(const FlatIvfRange& R, const uint32_t* s_val, const uint32_t* s_cnt, int s, int nqs,
                                                 bool list_read, int tid) {
    __syncthreads();
    if (tid < nqs) R.counts[s_val[s + tid]] = list_read ? (int64_t)s_cnt[tid] : 0;
}

// ---- the filled tile of a scan under an id filter -------------------------------------------------------
// A tile of a filtered scan is the next up to kFlatIvfTileRows ELIGIBLE rows of the list, not its next 256 row numbers.
// From list position `pos` on the workgroup reads row numbers in chunks of 256, a thread to a row number, and tests the
// row's bit in `fbits` (bit r & 31 of word r >> 5: the filter's bitmap over the handle's rows; every row number of a list is
// below the handle's row count, which the bitmap covers).  The survivors of a chunk are compacted in list order: a
// wavefront ballot gives a lane its place among its wavefront's survivors, the four wavefronts' counts -- through LDS --
// its wavefront's place in the chunk, and `fill` the chunk's place in the tile.  What fits goes to s_rows[place]; of what
// does not fit, the first survivor's thread leaves its offset in the chunk, and THERE the next tile's fill starts again:
// the carry is a list position, not a second row-number buffer, and costs the next tile at most one chunk read twice.
// Stops at a full tile or at the list's end; the slots behind the last row are kNoRow.  Returns the rows of the tile and
// moves pos to where the next tile starts; both are read from LDS behind a barrier, the same in every thread.
// Called by all 256 threads behind a barrier after which nobody reads s_rows; ends behind a barrier.  The words of two
// consecutive chunks alternate between two sets, so a chunk costs two barriers.
__device__ __forceinline__ int fill_tile(uint32_t* s_rows, const uint32_t* __restrict__ list_rows, int64_t& pos, int64_t hi,
                                         const uint32_t* __restrict__ fbits, int tid) {
    __shared__ uint32_t s_wcnt[2][4], s_stop[2];
    const int lane = tid & 63, w = tid >> 6;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    s_rows[tid] = kNoRow;
    uint32_t fill = 0u;
    for (int it = 0; fill < (uint32_t)kFlatIvfTileRows && pos < hi; it ^= 1) {
        const bool in = pos + tid < hi;
        const uint32_t row = in ? list_rows[pos + tid] : 0u;
        const bool ok = in && ((fbits[row >> 5] >> (row & 31u)) & 1u) != 0u;
        const uint64_t m = __ballot(ok);
        if (lane == 0) s_wcnt[it][w] = (uint32_t)__popcll(m);
        if (tid == 0) s_stop[it] = (uint32_t)kFlatIvfTileRows;  // the whole chunk, unless a survivor does not fit
        __syncthreads();  // also: s_rows is cleared before the first chunk's survivors land
        uint32_t before = 0u, total = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t c = s_wcnt[it][i];
            before += i < w ? c : 0u;
            total += c;
        }
        const uint32_t slot = fill + before + (uint32_t)__popcll(m & below);
        if (ok && slot < (uint32_t)kFlatIvfTileRows) s_rows[slot] = row;
        if (ok && slot == (uint32_t)kFlatIvfTileRows) s_stop[it] = (uint32_t)tid;  // one thread at most
        __syncthreads();
        pos += s_stop[it];
        fill = min(fill + total, (uint32_t)kFlatIvfTileRows);
    }
    return (int)fill;
}

}  // namespace
}  // namespace dpq

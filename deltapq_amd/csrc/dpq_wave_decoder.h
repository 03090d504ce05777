// dpq_wave_decoder.h -- internal device header: the delta decode of one 64-node chunk by one wavefront
// (Cfg, the byte-permute table and WaveDecoder), shared by dpq_kernels.hip (the scans, the per-batch decode) and
// dpq_lookup.hip (code lookup).  Every translation unit that includes it carries its own copy of g_dtab (4 KB).
#pragma once
#include "dpq_kernels.h"

namespace dpq {

__device__ __forceinline__ uint32_t bperm(int src_lane, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)v);
}

// number of set bits of a wave-uniform 64-bit mask strictly below this lane
__device__ __forceinline__ uint32_t mbcnt64(uint64_t m, uint32_t acc) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, acc));
}

// ---------------------------------------------------------------------------
// a5: delta decode of one 64-node chunk by one wavefront.
// M = 8: the reference format (a code is 2 dwords, 8 stack levels).
// M = 16: this build's extension (4 dwords, 2-byte masks, 16 levels); the
// reference format stops at M = 8 (h:1765, 1791-1795, 2883).
// ---------------------------------------------------------------------------

template <int M>
struct Cfg {
    static constexpr int W = M / 4;                   // dwords per code
    static constexpr int LEVELS = M <= 8 ? 8 : 16;    // ancestor stack entries (h:2858-2864: M of them)
    static constexpr int JUMPS = M <= 8 ? 3 : 4;      // pointer-jumping rounds: 2^JUMPS > deepest in-chunk chain
    static constexpr int PLANES = M <= 8 ? 4 : 5;     // bits of popcount(mask)
    // ---- filter tables of the scan ----
    static constexpr int EB = 8;                      // bits per table entry (4 queries per table dword)
    static constexpr int AB = M <= 8 ? 8 : 16;        // bits per field of the accumulators the entries are summed in
    static constexpr int R = AB / EB;                 // accumulator dwords per table dword
    static constexpr int F = 32 / AB;                 // fields (= queries) per accumulator dword
    static constexpr int NG = M <= 8 ? 4 : 2;         // 16-byte entries per (m, code): NG * M * 256 * 16 B = 128 KB
    static constexpr int NA = NG * 4 * R;             // accumulator dwords per node
    static constexpr int QG = NA * F;                 // queries per scan workgroup: 64 (M = 8), 32 (M = 16)
    static constexpr int J = NA < AB ? NA : AB;       // accumulator dwords folded into one survivor-mask dword
    static constexpr int MD = (NA + AB - 1) / AB;     // survivor-mask dwords per lane
    // 8-bit geometry re-swept on the GPU with bootstrap thresholds (QT/SAT -> exact checks per query, scan ms per
    // 1000 queries): 32/20 5644 0.198, 40/21 3848 0.178, 48/22 3004 0.169, 56/23 2585 0.165, 64/24 2413 0.163,
    // 80/26 2474 0.164, 90/26 3129 0.170, 100/27 3756 0.178, 120/30 4789 0.189 -- saturation costs more than resolution
    // M = 16: sixteen byte entries at that resolution do not fit a byte sum (QT 110 / SAT 31 with the top bits set
    // aside every four sub-spaces: 3.3 x the exact checks of 16-bit entries and a slower scan), and 16-bit ENTRIES
    // (round 1) serve 16 queries per decode pass at 32 LDS bytes per pair.  So the entries are bytes, summed four
    // sub-spaces at a time as bytes (4 * SAT <= 255) and then widened into 16-bit accumulator fields: 32 queries
    // per pass, 16 LDS bytes per pair.  Swept on the GPU (entries summed as bytes / SAT / QT -> exact checks per
    // query, M q/s at top-1000 and top-100; 16-bit entries: 7775, 0.995, 1.32): 4/63/160 17766 0.91 1.67,
    // 4/63/200 15134 0.99 1.77, 4/63/250 13776 1.04 1.79, 4/63/300 14271 1.02 1.75, 4/63/400 22002 0.81 1.46,
    // 2/127/200 15075 0.95 1.58, 1/255/320 11686 0.97 1.47, 1/255/400 10710 0.99 1.47 -- every unit of bound an
    // entry loses to rounding lets more of a concentrated 16-sub-space distance distribution through, but the
    // widening instructions of the finer geometries cost as much as the checks they save.
#ifndef DPQ_QT16
#define DPQ_QT16 250
#define DPQ_SAT16 63
#define DPQ_PRE16 4
#endif
    // M = 8 with the in-scan tightening's headroom (8 SAT + BIAS + XMAX XU <= 255), scripts/sim_filter_nibbles.py, survivors
    // per query at a threshold of rank 800 / 400 / 200: 80/26 (no headroom) 2241 / 1139 / 550, 64/24 (none) 2156 / 1066 /
    // 501, 64/22 2414 / 1211 / 574, 72/23 2515 / 1284 / 620, 80/23 3113 / 1639 / 818
    // Round 3, last step: tightening steps of ONE unit (seven steps = 11 % of the span; finer steps locate the cut better
    // than a longer range reaches, as at M = 16) free a unit of saturation: 64/23 with XU 1 against 64/22 with XU 2 on the
    // GPU (scripts/gpu_xu8.sh): exact checks per query 1676 against 1810 at top-100 (candidates 400 / 401), 12 514 against
    // 13 344 at top-1000; scan launch 0.1148 / 0.1178 ms and 0.284 / 0.298 ms.
    // Saturation per (slot, sub-space) (filter_saturations, dpq_kernels.hip): the saturations of a slot
    // share SAT_BUDGET = 122 + QT - XMAX XU + 1 units (210 at QT 88), split by the spread of the query's eight table
    // rows; the uniform split SAT_BUDGET / M (26 at QT 88; the sweeps above ran with one SAT for all, 23 at QT 64) is
    // the fallback of a slot without a scale.  With saturation no longer what a finer resolution costs, QT re-swept on
    // the GPU (profiles/filter_sat_sweep.txt; exact checks / candidates per query, scan ms per step, at top-100 and
    // top-1000; uniform 64/23: 1707 / 408, 0.1212 and 12 667 / 3779, 0.3060):
    // 64: 1514 / 410, 0.1196 and 11 909 / 3788, 0.2930;  72: 1416 / 422, 0.1181 and 11 099 / 3938, 0.2778;
    // 80: 1366 / 435, 0.1181 and 10 664 / 4107, 0.2701;  88: 1358 / 450, 0.1177 and 10 468 / 4280, 0.2655.
    // That sweep ran on an intermediate build whose bootstrap epilogue was 3 us longer than the one kept; checks,
    // candidates and scan times do not depend on the epilogue, step times do.  The headline (top-100) steps do not
    // tell the four values apart on either build, so the choice of 88 rests on top-1000 alone: fewest checks and
    // shortest step there (this build against the parent: 0.344 against 0.375 ms, profiles/filter_sat_ab.txt).
    // Candidates rise because seven tightening steps of one unit reach 8 % of the span at QT 88 where they reached
    // 11 % at QT 64.
#ifndef DPQ_QT8
#define DPQ_QT8 88
#endif
    static constexpr int QT = M <= 8 ? DPQ_QT8 : DPQ_QT16;   // filter units that span (tau - sum of minima)
    // In-scan tightening: a slot's cut can be lowered by e * XU filter units, e = 1 .. XMAX, while a scan launch runs
    // (the additive term of its accumulator field grows by as much): the field sums need that much headroom.
    static constexpr int XMAX = kTightBuckets - 1;
#ifndef DPQ_XU8
#define DPQ_XU8 1
#endif
#ifndef DPQ_XU16
#define DPQ_XU16 6  // swept on the GPU at top-1000 (scripts/gpu_xu16.sh; exact checks per query, ms per step): 4: 10823, 0.754; 6: 10295, 0.742; 8: 10806, 0.757; 12: 11957, 0.798; 16: 13133, 0.849; 24: 15919, 0.959 (top-100: 0.366 - 0.376)
#endif
    static constexpr int XU = M <= 8 ? DPQ_XU8 : DPQ_XU16;  // about a quarter of QT at XMAX steps: the k-th distance of a bootstrap
                                               // threshold of rank 8 k lies 17 % of (tau - minima) above the final one
    // field sum >= 2^(AB-1) (its top bit) <=> sum of entries > QT + 1.  R = 1: added to every m = 0 entry;
    // R = 2: the accumulator fields start from it.
    static constexpr int BIAS = (1 << (AB - 1)) - 1 - (QT + 1);
    static constexpr int FIELD_MAX = (1 << EB) - 1;
    // R = 1: what the M saturations of a slot may sum to (a byte field holds sum of SAT_m + BIAS + XMAX XU <= 255);
    // SAT: the uniform split, used where a slot has no scale.  R = 2: every entry saturates at DPQ_SAT16.
    static constexpr int SAT_BUDGET = R == 1 ? FIELD_MAX - BIAS - XMAX * XU : M * DPQ_SAT16;
    static constexpr int SAT = SAT_BUDGET / M;
    static constexpr int SAT_CAP = QT + 1;  // an entry above QT rejects alone: a larger saturation is wasted
    static_assert(BIAS >= 0 && SAT_BUDGET + BIAS + XMAX * XU < (1 << AB), "a field sum must not carry into its neighbour");
    static_assert(R != 1 || (SAT_BUDGET >= M && SAT_CAP <= 127 && M * SAT <= SAT_BUDGET), "saturations are 7-bit, one unit each at least");
    static_assert(XMAX * XU < QT, "cuts stay above zero");
    static constexpr int PRE = R == 1 ? M : DPQ_PRE16;  // entries summed as bytes before they are widened
    static_assert(R == 1 || (PRE * SAT <= FIELD_MAX && M * SAT > QT + 1 && M % PRE == 0), "byte sums of PRE entries; all-SAT rejects");
    static constexpr uint32_t LOW = AB == 8 ? 0x01010101u : 0x00010001u;  // bit 0 of every accumulator field
    // local slot of field f of accumulator dword acc: survivor-mask dword acc / AB, bit AB * f + acc % AB
    __host__ __device__ static constexpr int slot_of(int acc, int f) { return (acc / AB) * (J * F) + f * J + acc % AB; }
    // byte tb of dword c of 16-byte entry g of the tables <-> local slot: its accumulator is (4 g + c) R + tb % R
    // (R = 2: even bytes widen into one accumulator, odd bytes into the next), field tb / R
    __host__ __device__ static constexpr int slot_of_table(int g, int c, int tb) {
        return slot_of((4 * g + c) * R + tb % R, tb / R);
    }
    // the table entry of a slot nobody asks for: its field sum rejects every node
    __host__ __device__ static constexpr uint32_t reject_entry(int m) {
        return R == 1 ? (m == 0 ? (uint32_t)FIELD_MAX : 0u) : (uint32_t)SAT;
    }
    // refine queue of a wavefront: one entry per node with filter survivors = (code, id, survivor mask);
    // (16 wavefronts share what the 128 KB of tables and the tightening's 1-2 KB histogram leave of the 160 KB)
    static constexpr int QE_BYTES = 4 * W + 4 + 4 * MD;
    static constexpr int QCAP = M <= 8 ? 88 : 80;
    static_assert(QCAP >= 64 + 16, "a step pushes up to 64 entries");
};

// a7: the reference's decoder[256] (main:312-325) as byte-permute selectors.
// entry[0]/[1]: v_perm_b32 selectors that move a node's packed changed bytes to
// positions 0..3 / 4..7 of an 8-position group (0x0c = constant zero).
// A compile-time table in global memory (4 KB, lives in the vector L1): the
// scan is bound by LDS cycles, so the decode keeps its table out of the LDS.
struct DecodeTable {
    uint32_t e[256][2];
    constexpr DecodeTable() : e() {
        for (int b = 0; b < 256; ++b) {
            uint32_t sel[2] = {0, 0};
            uint32_t rank = 0;
            for (int m = 0; m < 8; ++m) {
                const bool set = (b >> m) & 1;
                sel[m >> 2] |= (set ? rank : 0x0cu) << (8 * (m & 3));
                rank += set ? 1u : 0u;
            }
            e[b][0] = sel[0];
            e[b][1] = sel[1];
        }
    }
};
__device__ const DecodeTable g_dtab{};

// bit i (0..3) of `nib` -> v_perm_b32 selector byte i: i (take the own byte) where the bit is set,
// 4 + i (take the other operand's byte) elsewhere.  perm(other, own, sel).
__device__ __forceinline__ uint32_t own_sel(uint32_t nib) {
    return 0x07060504u - ((nib * 0x00810204u) & 0x04040404u);  // nib < 16: bit i lands on bit 8 i + 2, no carries
}

template <int M>
struct WaveDecoder {
    static constexpr int W = Cfg<M>::W;
    static constexpr int LEVELS = Cfg<M>::LEVELS;
    uint32_t stk[W];  // ancestor stack (vecs_stack, h:2858-2862) in lanes 0..LEVELS-1
    uint64_t doff;    // offset of the chunk's first changed byte

    __device__ __forceinline__ void begin_segment(const DeviceImage& img, uint32_t seg, int lane) {
        doff = img.seg_delta_off[seg];
#pragma unroll
        for (int w = 0; w < W; ++w) stk[w] = 0;
        if (lane < LEVELS) {
            const uint32_t* ck = reinterpret_cast<const uint32_t*>(img.seg_ckpt) + ((size_t)seg * LEVELS + lane) * W;
#pragma unroll
            for (int w = 0; w < W; ++w) stk[w] = ck[w];
        }
    }

    // The decode of a 64-node chunk runs in three stages so that the scan can keep the stages of three
    // consecutive chunks in flight (each of the first two ends in a global-memory round trip):
    //   load_in   depth nibble and diff mask of the lane's node (coalesced)
    //   load_delta wave scan of popcount(mask) -> the node's changed bytes (3 aligned dwords) + permute selectors
    //   finish    scatter to positions, pointer jumping over the in-chunk ancestor chain, apply to the stack
    struct In {
        uint32_t nb, mk, par;
    };
    struct Ld {
        uint32_t level, mk, par;
        uint32_t w[W / 2][3], sh[W / 2];
        uint2 t[W / 2];
    };
    __device__ __forceinline__ static In load_in(const DeviceImage& img, int64_t node) {
        In r;
        r.nb = img.nib[node >> 1];
        r.mk = M <= 8 ? (uint32_t)img.mask[node] : (uint32_t)reinterpret_cast<const uint16_t*>(img.mask)[node];
        r.par = img.par[node];
        return r;
    }
    // `at`: running offset of the chunk's first changed byte (advanced past the chunk)
    __device__ __forceinline__ static Ld load_delta(const DeviceImage& img, const In& in, int64_t node, uint64_t& at) {
        Ld r;
        r.level = (node & 1) ? (in.nb >> 4) : (in.nb & 15u);
        r.mk = in.mk;
        r.par = in.par;
        const uint32_t pc = __popc(in.mk);
        // wave exclusive scan of pc by bit planes: v_mbcnt, no LDS traffic
        uint32_t excl = 0, total = 0;
#pragma unroll
        for (int b = Cfg<M>::PLANES - 1; b >= 0; --b) {
            const uint64_t plane = __ballot((pc >> b) & 1u);
            excl = mbcnt64(plane, excl << 1);
            total = (total << 1) + (uint32_t)__popcll(plane);
        }
        // changed bytes at byte granularity, one 8-position group at a time: 3 aligned dwords (+ funnel shift later)
#pragma unroll
        for (int h = 0; h < W / 2; ++h) {
            const uint32_t skip = h == 0 ? 0u : (uint32_t)__popc(in.mk & 0xffu);
            const uint8_t* dp = img.delta + at + excl + skip;
            const uintptr_t ua = reinterpret_cast<uintptr_t>(dp);
            const uint32_t* wp = reinterpret_cast<const uint32_t*>(ua & ~(uintptr_t)3);
            r.sh[h] = (uint32_t)(ua & 3);
            r.w[h][0] = wp[0];
            r.w[h][1] = wp[1];
            r.w[h][2] = wp[2];
            r.t[h] = *reinterpret_cast<const uint2*>(g_dtab.e[(in.mk >> (8 * h)) & 0xffu]);
        }
        at += total;
        return r;
    }

    // Decode node `node` (= this lane's node of the chunk) in one go.  `carry`: update the
    // stack for the next chunk of the segment.
    __device__ __forceinline__ void step(const DeviceImage& img, int64_t node, int lane, bool carry, uint32_t (&code)[W]) {
        const In in = load_in(img, node);
        const Ld ld = load_delta(img, in, node, doff);
        uint32_t cl = 0xffu;
        if (carry && lane < LEVELS) cl = img.carry[(size_t)(node >> 6) * LEVELS + lane];
        finish(ld, lane, cl, code);
    }

    // carry_lane (lanes 0..LEVELS-1): lane of the chunk's last node of depth `lane`, 0xFF = none / no carry wanted
    __device__ __forceinline__ void finish(const Ld& ld, int lane, uint32_t carry_lane, uint32_t (&code)[W]) {
        uint32_t mk = ld.mk;
        uint32_t pv[W];
#pragma unroll
        for (int h = 0; h < W / 2; ++h) {  // scatter the packed changed bytes to their positions (a7)
            const uint32_t raw_lo = __builtin_amdgcn_alignbyte(ld.w[h][1], ld.w[h][0], ld.sh[h]);
            const uint32_t raw_hi = __builtin_amdgcn_alignbyte(ld.w[h][2], ld.w[h][1], ld.sh[h]);
            pv[2 * h] = __builtin_amdgcn_perm(raw_hi, raw_lo, ld.t[h].x);
            pv[2 * h + 1] = __builtin_amdgcn_perm(raw_hi, raw_lo, ld.t[h].y);
        }
        // parent = nearest preceding node with depth - 1 (h:2888: stack[depth-1]); which lane that is was
        // resolved when the image was built (DeviceImage::par), as was the stack level the chain ends on
        uint32_t P = ld.par;  // 0xFF: the parent precedes the chunk
        // Pointer jumping: compose patches along the in-chunk ancestor chain.  A patch travels as its
        // W value dwords plus ONE dword (position mask | parent lane): the byte selectors that merge two
        // patches are rebuilt from the position mask (VALU) instead of being carried through the LDS
        // crossbar -- the scan is bound by LDS cycles.
#pragma unroll
        for (int s = 0; s < Cfg<M>::JUMPS; ++s) {
            if (__ballot(P != 0xffu) == 0) break;  // every chain is resolved (wave-uniform)
            const int src = P == 0xffu ? lane : (int)P;
            uint32_t q_pv[W];
#pragma unroll
            for (int w = 0; w < W; ++w) q_pv[w] = bperm(src, pv[w]);
            const uint32_t q_meta = bperm(src, mk | (P << 16));
            if (P != 0xffu) {
#pragma unroll
                for (int w = 0; w < W; ++w) pv[w] = __builtin_amdgcn_perm(q_pv[w], pv[w], own_sel((mk >> (4 * w)) & 15u));
                mk |= q_meta & 0xffffu;
                P = q_meta >> 16;
            }
        }
        // apply to the ancestor that precedes the chunk
#pragma unroll
        for (int w = 0; w < W; ++w)
            code[w] = __builtin_amdgcn_perm(bperm((int)ld.level, stk[w]), pv[w], own_sel((mk >> (4 * w)) & 15u));
        // carry the stack: stack[D] = code of the last node with depth D
        if (__ballot(carry_lane != 0xffu)) {
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const uint32_t nv = bperm(carry_lane == 0xffu ? lane : (int)carry_lane, code[w]);
                if (carry_lane != 0xffu) stk[w] = nv;
            }
        }
    }
};

}  // namespace dpq

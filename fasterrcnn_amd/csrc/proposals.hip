// proposals.hip -- RPN proposal generation without host round trips.
// Replaces, in order (reference: models/rpn.py):
//   :89  t.sigmoid                          \
//   :98-104,158-173 _extract_valid            >  rpn_decode_kernel (one thread per anchor)
//   :118-123 t_convert_deltas_to_boxes      /   (models/math_utils.py:122-127, fp32, no FMA)
//   :129-132 argsort ascending, flip, [0:N]    topk_sort_kernel: 8-pass radix select of the
//                                              N-th largest 64-bit key, LDS bitonic sort of the
//                                              survivors.  key = (score bits, anchor index+1):
//                                              unique keys -> one deterministic order; ties go
//                                              to the HIGHER anchor index, which is what a stable
//                                              ascending sort followed by flip() produces.
//   :135-144 clamp, >= 16 px filter            same kernel, order-preserving scan compaction
//   :147-153 torchvision.ops.nms(0.7)[0:N]     nms_mask_kernel (64x64 IoU bit tiles) +
//                                              nms_reduce_kernel (one wave: 64 boxes per step,
//                                              readlane over the diagonal word, a band of
//                                              look-ahead words per row, early exit); in two
//                                              phases: the mask's leading NMS_BAND column chunks
//                                              first, the rest only if the list needs them
#include "geometry.h"
#include <type_traits>

namespace frcnn {

typedef unsigned long long u64;

__device__ __forceinline__ unsigned ordered_bits(float f)
{
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float from_ordered_bits(unsigned o)
{
    const unsigned b = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    return __uint_as_float(b);
}

// One thread per anchor n = (y*fw + x)*9 + k  (the reference's flat order, rpn.py:162-165).
__global__ __launch_bounds__(256)
void rpn_decode_kernel(const float* __restrict__ head, int ld, const float* __restrict__ anchors,
                       const float* __restrict__ valid, int A, float* __restrict__ scores,
                       f32x4* __restrict__ boxes_all, u64* __restrict__ keys)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= A) return;
    const int pix = n / 9, k = n - pix * 9;
    const float* row = head + (size_t)pix * ld;
    const float logit = row[k];
    const float score = 1.0f / (1.0f + expf(-logit));
    const float dy = row[9 + 4 * k + 0], dx = row[9 + 4 * k + 1];
    const float dh = row[9 + 4 * k + 2], dw = row[9 + 4 * k + 3];
    const f32x4 a = reinterpret_cast<const f32x4*>(anchors)[n];   // cy, cx, h, w
    // center = anchors[:,2:4] * deltas[:,0:2] + anchors[:,0:2]  (two roundings, as torch does)
    const float cy = __fadd_rn(__fmul_rn(a[2], dy), a[0]);
    const float cx = __fadd_rn(__fmul_rn(a[3], dx), a[1]);
    const float h = __fmul_rn(a[2], expf(dh));
    const float w = __fmul_rn(a[3], expf(dw));
    const float hh = 0.5f * h, hw = 0.5f * w;
    f32x4 b;
    b[0] = cy - hh; b[1] = cx - hw; b[2] = cy + hh; b[3] = cx + hw;
    scores[n] = score;
    boxes_all[n] = b;
    const bool ok = (valid == nullptr) || (valid[n] > 0.f);
    keys[n] = ok ? (((u64)ordered_bits(score) << 32) | (u64)(unsigned)(n + 1)) : 0ull;
}

// keys for the stand-alone NMS entry: stable descending (ties -> LOWER index first), the order of the oracle's stable
// argsort(-scores): -0.0 ties with +0.0 (the score bits alone would put +0.0 above it), and every NaN gets the lowest score key, 0, so
// NaNs sort after -inf, among themselves by index.  (No non-NaN float maps to 0: -inf is 0x007FFFFF.)
__global__ __launch_bounds__(256)
void nms_keys_kernel(const float* __restrict__ scores, int n, u64* __restrict__ keys)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float f = scores[i];
    const unsigned hi = f != f ? 0u : ordered_bits(f == 0.f ? 0.f : f);
    keys[i] = ((u64)hi << 32) | (u64)(0xFFFFFFFFu - (unsigned)i);
}

// ---- register-resident bitonic sort (descending) of 1024*PER keys held PER-per-thread ---------------
// thread t owns global positions [PER*t, PER*t+PER).  Sub-passes with partner distance j < PER are
// in-thread, PER <= j < 64*PER go through __shfl_xor (same wave), j >= 64*PER through LDS.
__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int lane_mask)
{
    const unsigned lo = __shfl_xor((unsigned)(v & 0xFFFFFFFFull), lane_mask);
    const unsigned hi = __shfl_xor((unsigned)(v >> 32), lane_mask);
    return ((u64)hi << 32) | lo;
}

// element at global index g, partner at g ^ j, run length k: keep max iff (descending run) == (lower index)
__device__ __forceinline__ u64 bitonic_pick(u64 mine, u64 other, int g, int j, int k)
{
    const bool keep_max = (((g & k) == 0) == ((g & j) == 0));
    const bool other_bigger = other > mine;
    return (keep_max == other_bigger) ? other : mine;
}

template <int PER, int J>
__device__ __forceinline__ void bitonic_inthread(u64 (&e)[PER], int base, int k)
{
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        if ((r & J) == 0) {
            const u64 a = e[r], b = e[r | J];
            e[r] = bitonic_pick(a, b, base + r, J, k);
            e[r | J] = bitonic_pick(b, a, base + (r | J), J, k);
        }
    }
}

template <int PER>
__device__ void bitonic_sort_regs(u64* buf, int tid)
{
    constexpr int N = 1024 * PER;
    u64 e[PER];
    const int base = tid * PER;
#pragma unroll
    for (int r = 0; r < PER; ++r) e[r] = buf[base + r];
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j >= 64 * PER) {
#pragma unroll
                for (int r = 0; r < PER; ++r) buf[base + r] = e[r];
                __syncthreads();
#pragma unroll
                for (int r = 0; r < PER; ++r) e[r] = bitonic_pick(e[r], buf[(base + r) ^ j], base + r, j, k);
                __syncthreads();
            } else if (j >= PER) {
                const int lane_mask = j / PER;
#pragma unroll
                for (int r = 0; r < PER; ++r) e[r] = bitonic_pick(e[r], shfl_xor_u64(e[r], lane_mask), base + r, j, k);
            } else {
                if (PER > 8 && j == 8) bitonic_inthread<PER, (PER > 8 ? 8 : 1)>(e, base, k);
                else if (PER > 4 && j == 4) bitonic_inthread<PER, (PER > 4 ? 4 : 1)>(e, base, k);
                else if (PER > 2 && j == 2) bitonic_inthread<PER, (PER > 2 ? 2 : 1)>(e, base, k);
                else if (PER > 1 && j == 1) bitonic_inthread<PER, 1>(e, base, k);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < PER; ++r) buf[base + r] = e[r];
    __syncthreads();
}

// Single block, 1024 threads.  Selects the K largest of n_keys 64-bit keys (zero keys are
// "absent"), sorts them descending in LDS, then emits them.
//   MODE 0 (RPN): idx = low-1; writes sorted_idx; clips to the image, drops boxes with a side
//                 < min_side, compacts in order into cand_boxes/cand_scores.
//   MODE 1 (NMS): idx = 0xFFFFFFFF-low; gathers boxes in sorted order, no clip/filter.
// counts[0] = number selected (<= K), counts[1] = number emitted to cand_*.
//   SPLIT (round 3, MODE 0 only): the kernel stops after the radix select: the survivors go, unsorted, to `sel_out` (sort_n keys, zero
//   padded), counts[0] = their number; topk_rank_kernel (many blocks) and topk_emit_kernel finish the job.  The one-block register
//   bitonic sort of 8192 keys was 63 of this kernel's 103 us with the rest of the chip idle.
template <int MODE, bool SPLIT = false>
__global__ __launch_bounds__(1024)
void topk_sort_kernel(const u64* __restrict__ keys, int n_keys, int K, int sort_n,
                      const f32x4* __restrict__ boxes_src, float image_h, float image_w, float min_side,
                      int32_t* __restrict__ sorted_idx, f32x4* __restrict__ cand_boxes,
                      float* __restrict__ cand_scores, int32_t* __restrict__ counts, u64* __restrict__ sel_out = nullptr)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u64* buf = reinterpret_cast<u64*>(smem_raw);                 // [sort_n]
    int* hist = reinterpret_cast<int*>(buf + sort_n);            // [4096]
    int* misc = hist + 4096;                                     // [64]
    const int tid = threadIdx.x;

    // each thread keeps its keys (i = tid + 1024*it) in registers when they fit: the select reads them 8 times
    constexpr int KPT = 24;
    const bool in_regs = n_keys <= 1024 * KPT;
    u64 kreg[KPT];
#pragma unroll
    for (int it = 0; it < KPT; ++it) {
        const int i = tid + 1024 * it;
        kreg[it] = (in_regs && i < n_keys) ? keys[i] : 0ull;
    }

#ifdef TOPK_CLOCKS
    unsigned long long tk[6]; tk[0] = __builtin_readcyclecounter();
#endif
    // ---- how many keys are present ----------------------------------------------------------
    if (tid == 0) { misc[0] = 0; misc[1] = 0; }
    __syncthreads();
    {
        int c = 0;
        if (in_regs) {
#pragma unroll
            for (int it = 0; it < KPT; ++it) c += kreg[it] != 0ull;
        } else {
            for (int i = tid; i < n_keys; i += 1024) c += keys[i] != 0ull;
        }
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if ((tid & 63) == 0 && c) atomicAdd(&misc[0], c);
    }
    __syncthreads();
    const int present = misc[0];
    const int want = present < K ? present : K;
    __syncthreads();

#ifdef TOPK_CLOCKS
    tk[1] = __builtin_readcyclecounter();
#endif
    // ---- radix select: threshold = want-th largest key --------------------------------------
    // 12-bit digits (4096 bins): four histogram passes over the 48 significant bits of an RPN key instead of six 8-bit ones, and
    // the scores' clustered high bits spread over 16x more bins -- the LDS atomics of a pass serialise per address.
    u64 thr = 1ull;            // all present keys
    if (present > K) {
        u64 prefix = 0ull, pmask = 0ull;
        int remaining = K;
        const bool short_idx = MODE == 0 && n_keys < 65535;        // index + 1 < 2^16: bits 31..16 are 0 in every key
        // digit d covers bits [sh, sh + bits)
        const int nd = short_idx ? 5 : 6;
        for (int d = 0; d < nd; ++d) {
            int sh, bits;
            if (short_idx) { sh = d == 0 ? 52 : d == 1 ? 40 : d == 2 ? 32 : d == 3 ? 4 : 0; bits = d == 2 ? 8 : d == 4 ? 4 : 12; }
            else { sh = d == 0 ? 52 : d == 1 ? 40 : d == 2 ? 28 : d == 3 ? 16 : d == 4 ? 4 : 0; bits = d == 5 ? 4 : 12; }
            const int nb = 1 << bits;
            const u64 dmask = (u64)(nb - 1);
            for (int i = tid; i < nb; i += 1024) hist[i] = 0;
            __syncthreads();
            if (in_regs) {
#pragma unroll
                for (int it = 0; it < KPT; ++it) {
                    const u64 k = kreg[it];
                    if (k != 0ull && (k & pmask) == prefix) atomicAdd(&hist[(int)((k >> sh) & dmask)], 1);
                }
            } else {
                for (int i = tid; i < n_keys; i += 1024) {
                    const u64 k = keys[i];
                    if (k != 0ull && (k & pmask) == prefix) atomicAdd(&hist[(int)((k >> sh) & dmask)], 1);
                }
            }
            __syncthreads();
            {
                // thread t owns bins top .. top - 3 (descending); block-wide inclusive scan of the counts from the top bin down
                const int top = nb - 1 - 4 * tid;
                const bool own = top >= 3;
                const int h0 = own ? hist[top] : 0, h1 = own ? hist[top - 1] : 0, h2 = own ? hist[top - 2] : 0, h3 = own ? hist[top - 3] : 0;
                const int sum = h0 + h1 + h2 + h3;
                int incl = sum;
                for (int o = 1; o < 64; o <<= 1) {
                    const int v = __shfl_up(incl, o);
                    if ((tid & 63) >= o) incl += v;
                }
                if ((tid & 63) == 63) misc[8 + (tid >> 6)] = incl;
                __syncthreads();
                int off = 0;
                for (int wv = 0; wv < (tid >> 6); ++wv) off += misc[8 + wv];
                incl += off;
                const int excl = incl - sum;
                if (excl < remaining && incl >= remaining) {       // exactly one thread
                    int c = excl, dg = top;
                    if (c + h0 < remaining) { c += h0; dg = top - 1;
                        if (c + h1 < remaining) { c += h1; dg = top - 2;
                            if (c + h2 < remaining) { c += h2; dg = top - 3; } } }
                    misc[2] = dg; misc[3] = remaining - c;
                }
            }
            __syncthreads();
            prefix |= (u64)misc[2] << sh;
            pmask |= dmask << sh;
            remaining = misc[3];
            __syncthreads();
        }
        if (short_idx) pmask |= 0xFFFF0000ull;                      // (all zero)
        thr = prefix;
    }

#ifdef TOPK_CLOCKS
    tk[2] = __builtin_readcyclecounter();
#endif
    // ---- gather survivors into LDS, pad, bitonic sort descending -----------------------------
    for (int i = tid; i < sort_n; i += 1024) buf[i] = 0ull;
    __syncthreads();
    if (in_regs) {
        // one returning atomic per wave and round instead of one per survivor (6000 on one address); the order inside buf is
        // irrelevant, it is sorted next
#pragma unroll
        for (int it = 0; it < KPT; ++it) {
            const u64 k = kreg[it];
            const bool take = k != 0ull && k >= thr;
            const unsigned long long m = __ballot(take);
            if (m != 0ull) {
                const int lead = __ffsll((long long)m) - 1;
                int base = 0;
                if ((tid & 63) == lead) base = atomicAdd(&misc[1], __popcll(m));
                base = __shfl(base, lead);
                const int pos = base + __popcll(m & ((1ull << (tid & 63)) - 1ull));
                if (take && pos < sort_n) buf[pos] = k;
            }
        }
    } else {
        for (int i = tid; i < n_keys; i += 1024) {
            const u64 k = keys[i];
            if (k != 0ull && k >= thr) {
                const int pos = atomicAdd(&misc[1], 1);
                if (pos < sort_n) buf[pos] = k;
            }
        }
    }
    __syncthreads();
#ifdef TOPK_CLOCKS
    tk[3] = __builtin_readcyclecounter();
#endif
    if (SPLIT) {
        for (int i = tid; i < sort_n; i += 1024) sel_out[i] = buf[i];
        if (tid == 0) counts[0] = want;
        return;
    }
    if (sort_n == 8192) {
        bitonic_sort_regs<8>(buf, tid);          // the 6000-of-20646 case: 81 of 91 sub-passes barrier-free
    } else if (sort_n == 16384) {
        bitonic_sort_regs<16>(buf, tid);
    } else {
        for (int k = 2; k <= sort_n; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (sort_n >> 1); t += 1024) {
                    const int i = 2 * t - (t & (j - 1));
                    const int l = i + j;
                    const bool desc = (i & k) == 0;
                    const u64 a = buf[i], b = buf[l];
                    if ((a < b) == desc) { buf[i] = b; buf[l] = a; }
                }
                __syncthreads();
            }
        }
    }

#ifdef TOPK_CLOCKS
    tk[4] = __builtin_readcyclecounter();
#endif
    // ---- emit in rank order ------------------------------------------------------------------
    // thread t owns ranks [t*per, (t+1)*per).  With `per` a compile-time constant the box gathers of a thread are issued together
    // and kept for the second pass (they were 2 x per dependent global round trips).
    const int per = sort_n >> 10 ? sort_n >> 10 : 1;
    int* wave_tot = misc + 8;     // [16]
    int pos = 0;
    auto emit = [&](auto perc) {
        constexpr int PERC = decltype(perc)::value;
        u64 kk[PERC];
        f32x4 bb[PERC];
        bool kp[PERC];
        int local = 0;
#pragma unroll
        for (int q = 0; q < PERC; ++q) {
            const int p = tid * PERC + q;
            kp[q] = p < want && p < sort_n;
            kk[q] = kp[q] ? buf[p] : 0ull;
        }
#pragma unroll
        for (int q = 0; q < PERC; ++q) {
            const unsigned low = (unsigned)(kk[q] & 0xFFFFFFFFull);
            const int idx = MODE == 0 ? (int)(low - 1u) : (int)(0xFFFFFFFFu - low);
            bb[q] = kp[q] ? boxes_src[idx] : f32x4{0.f, 0.f, 0.f, 0.f};
            if (kp[q] && sorted_idx) sorted_idx[tid * PERC + q] = idx;
        }
#pragma unroll
        for (int q = 0; q < PERC; ++q) {
            if (MODE == 0) {
                f32x4 b = bb[q];
                b[0] = fmaxf(b[0], 0.f); b[1] = fmaxf(b[1], 0.f);
                b[2] = fminf(b[2], image_h); b[3] = fminf(b[3], image_w);
                bb[q] = b;
                kp[q] = kp[q] && ((b[2] - b[0]) >= min_side) && ((b[3] - b[1]) >= min_side);
            }
            local += kp[q];
        }
        // block exclusive scan of `local`
        int incl = local;
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o);
            if ((tid & 63) >= o) incl += v;
        }
        if ((tid & 63) == 63) wave_tot[tid >> 6] = incl;
        __syncthreads();
        int wave_off = 0;
        for (int wv = 0; wv < (tid >> 6); ++wv) wave_off += wave_tot[wv];
        pos = wave_off + incl - local;
#pragma unroll
        for (int q = 0; q < PERC; ++q) {
            if (kp[q]) {
                cand_boxes[pos] = bb[q];
                cand_scores[pos] = from_ordered_bits((unsigned)(kk[q] >> 32));
                ++pos;
            }
        }
    };
    if (per == 8) {
        emit(std::integral_constant<int, 8>());
    } else if (per == 16) {
        emit(std::integral_constant<int, 16>());
    } else {
        int local = 0;
        for (int q = 0; q < per; ++q) {
            const int p = tid * per + q;
            if (p < want && p < sort_n) {
                const u64 k = buf[p];
                const unsigned low = (unsigned)(k & 0xFFFFFFFFull);
                const int idx = MODE == 0 ? (int)(low - 1u) : (int)(0xFFFFFFFFu - low);
                if (sorted_idx) sorted_idx[p] = idx;
                if (MODE == 0) {
                    f32x4 b = boxes_src[idx];
                    b[0] = fmaxf(b[0], 0.f); b[1] = fmaxf(b[1], 0.f);
                    b[2] = fminf(b[2], image_h); b[3] = fminf(b[3], image_w);
                    const bool keep = ((b[2] - b[0]) >= min_side) && ((b[3] - b[1]) >= min_side);
                    local += keep;
                } else {
                    local += 1;
                }
            }
        }
        int incl = local;
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o);
            if ((tid & 63) >= o) incl += v;
        }
        if ((tid & 63) == 63) wave_tot[tid >> 6] = incl;
        __syncthreads();
        int wave_off = 0;
        for (int wv = 0; wv < (tid >> 6); ++wv) wave_off += wave_tot[wv];
        pos = wave_off + incl - local;
        for (int q = 0; q < per; ++q) {
            const int p = tid * per + q;
            if (p < want && p < sort_n) {
                const u64 k = buf[p];
                const unsigned low = (unsigned)(k & 0xFFFFFFFFull);
                const int idx = MODE == 0 ? (int)(low - 1u) : (int)(0xFFFFFFFFu - low);
                f32x4 b = boxes_src[idx];
                bool keep = true;
                if (MODE == 0) {
                    b[0] = fmaxf(b[0], 0.f); b[1] = fmaxf(b[1], 0.f);
                    b[2] = fminf(b[2], image_h); b[3] = fminf(b[3], image_w);
                    keep = ((b[2] - b[0]) >= min_side) && ((b[3] - b[1]) >= min_side);
                }
                if (keep) {
                    cand_boxes[pos] = b;
                    cand_scores[pos] = from_ordered_bits((unsigned)(k >> 32));
                    ++pos;
                }
            }
        }
    }
    if (tid == 1023) { counts[0] = want; counts[1] = pos; }
#ifdef TOPK_CLOCKS
    tk[5] = __builtin_readcyclecounter();
    if (tid == 0 && n_keys > 20000) printf("topk cycles: load %llu  select %llu  gather %llu  sort %llu  emit %llu\n", tk[1] - tk[0], tk[2] - tk[1], tk[3] - tk[2], tk[4] - tk[3], tk[5] - tk[4]);
#endif
}

// Rank sort of the selected keys (all different: the low word is the anchor index): rank = number of keys greater.  Block = 32 keys x 32
// segments of the list (1024 threads): wave w holds the keys 32 b .. 32 b + 31 twice (lane halves) against the segments 2 w and 2 w + 1, so
// that every LDS read of the inner loop is a broadcast; the 32 partial counts of a key meet in LDS.  The thread that owns a key then
// writes everything the old kernel's emit phase produced for its rank: sorted_idx, the clipped box, the score and the keep flag of the
// 16-pixel filter (models/rpn.py:135-144).  ~190 blocks for 6000 keys: the whole chip for a few microseconds.
__global__ __launch_bounds__(1024)
void topk_rank_kernel(const u64* __restrict__ sel, const int32_t* __restrict__ counts, int sort_n, const f32x4* __restrict__ boxes_src,
                      float image_h, float image_w, float min_side, int32_t* __restrict__ sorted_idx, f32x4* __restrict__ tmp_boxes,
                      float* __restrict__ tmp_scores, int32_t* __restrict__ keep_flag)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_rank[];
    u64* lk = reinterpret_cast<u64*>(smem_rank);                    // [sort_n]
    int* part = reinterpret_cast<int*>(lk + sort_n);               // [32 keys][32 segments]
    const int n = counts[0];
    const int k0 = blockIdx.x * 32;
    if (k0 >= n) return;
    const int tid = threadIdx.x;
    const int npad = (n + 31) & ~31;
    for (int i = tid; i < npad; i += 1024) lk[i] = i < n ? sel[i] : 0ull;
    __syncthreads();
    const int kb = tid & 31, seg = tid >> 5;                         // 32 segments
    const int seg_len = npad >> 5;
    const u64 mine = k0 + kb < n ? lk[k0 + kb] : ~0ull;
    const u64* p = lk + seg * seg_len;
    int cnt = 0;
    int j = 0;
    for (; j + 4 <= seg_len; j += 4) {
        const u64 a = p[j], b = p[j + 1], c = p[j + 2], d = p[j + 3];
        cnt += (a > mine) + (b > mine) + (c > mine) + (d > mine);
    }
    for (; j < seg_len; ++j) cnt += p[j] > mine;
    part[kb * 32 + seg] = cnt;
    __syncthreads();
    if (tid < 32 && k0 + tid < n) {
        int rank = 0;
#pragma unroll
        for (int q = 0; q < 32; ++q) rank += part[tid * 32 + ((q + tid) & 31)];        // rotated: conflict-free column walk
        const u64 k = lk[k0 + tid];
        const int idx = (int)((unsigned)(k & 0xFFFFFFFFull) - 1u);
        f32x4 b = boxes_src[idx];
        b[0] = fmaxf(b[0], 0.f); b[1] = fmaxf(b[1], 0.f);
        b[2] = fminf(b[2], image_h); b[3] = fminf(b[3], image_w);
        if (sorted_idx) sorted_idx[rank] = idx;
        tmp_boxes[rank] = b;
        tmp_scores[rank] = from_ordered_bits((unsigned)(k >> 32));
        keep_flag[rank] = (((b[2] - b[0]) >= min_side) && ((b[3] - b[1]) >= min_side)) ? 1 : 0;
    }
}

// Order-preserving compaction of the ranked candidates that passed the size filter: one block, thread t owns the ranks
// [t per, (t + 1) per).  counts[1] = number emitted.
__global__ __launch_bounds__(1024)
void topk_emit_kernel(const f32x4* __restrict__ tmp_boxes, const float* __restrict__ tmp_scores, const int32_t* __restrict__ keep_flag,
                      int sort_n, f32x4* __restrict__ cand_boxes, float* __restrict__ cand_scores, int32_t* __restrict__ counts)
{
    __shared__ int wave_tot[16];
    const int tid = threadIdx.x;
    const int n = counts[0];
    // flags, boxes and scores of the thread's ranks are all requested before anything is used: ONE global round trip
    auto body = [&](auto perc) {
        constexpr int PER = decltype(perc)::value;
        int fl[PER];
        f32x4 bx[PER];
        float sc[PER];
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int r = tid * PER + q;
            const bool in = r < n;
            fl[q] = in ? keep_flag[r] : 0;
            bx[q] = in ? tmp_boxes[r] : f32x4{0.f, 0.f, 0.f, 0.f};
            sc[q] = in ? tmp_scores[r] : 0.f;
        }
        int local = 0;
#pragma unroll
        for (int q = 0; q < PER; ++q) local += fl[q] ? 1 : 0;
        int incl = local;
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o);
            if ((tid & 63) >= o) incl += v;
        }
        if ((tid & 63) == 63) wave_tot[tid >> 6] = incl;
        __syncthreads();
        int wave_off = 0;
        for (int wv = 0; wv < (tid >> 6); ++wv) wave_off += wave_tot[wv];
        int pos = wave_off + incl - local;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            if (fl[q]) {
                cand_boxes[pos] = bx[q];
                cand_scores[pos] = sc[q];
                ++pos;
            }
        }
        if (tid == 1023) counts[1] = pos;
    };
    const int per = sort_n >> 10 ? sort_n >> 10 : 1;
    if (per == 8) body(std::integral_constant<int, 8>());
    else if (per == 16) body(std::integral_constant<int, 16>());
    else if (per == 4) body(std::integral_constant<int, 4>());
    else if (per == 2) body(std::integral_constant<int, 2>());
    else body(std::integral_constant<int, 1>());
}

// The NMS runs in two phases where the kept list is short against the candidate list.  nms_reduce_kernel stops at the chunk in which
// the last box is kept, and reads nothing of a row or a column behind it: on the workload's lists (6000 candidates, 300 kept) that is
// chunk 15 to 19 of 94, i.e. about 200 of the 4465 tiles on or above the diagonal (profiles/r08/nms_band.txt).  So
//   phase A: the mask's leading band, column chunks [0, NMS_BAND), and a reduce that may resolve NMS_BAND chunks.  If it keeps
//            max_keep boxes, or runs out of boxes, it writes the outputs and sets the `done` word (ProposalScratch::keep[0]: written by
//            every phase-A reduce, never cleared by the host);
//   phase B: the other columns, [NMS_BAND, nw), with every row chunk by <= bx, and the whole reduce again from chunk 0.  Both launches
//            read `done` first and return at once where it is set: a few microseconds of empty launches on every list the band covers,
//            and the full cost (plus phase A's reduce) only on a list that keeps its boxes later than any measured one.
// NMS_BAND = the smallest multiple of 8 that is >= 1.5 x the largest stopping chunk seen over the golden image, the hold-out images and
// the benchmark's pool (19: tools/nms_band.py, profiles/r08/nms_band.txt).
static constexpr int NMS_BAND = 32;

__host__ __device__ __forceinline__ int nms_tri(int k) { return k * (k + 1) / 2; }       // tiles with by <= bx < k

// One wave per 64x64 tile, over a one-dimensional grid of exactly the tiles with by <= bx and bx in [bx_begin, bx_end): block t is
// tile number nms_tri(bx_begin) + t in column-major order (column bx holds tiles nms_tri(bx) .. nms_tri(bx + 1) - 1, by ascending).
// `done` != NULL and *done != 0: the list is already reduced, nothing is read or written.
__global__ __launch_bounds__(64)
void nms_mask_kernel(const f32x4* __restrict__ boxes, const int32_t* __restrict__ n_ptr, float thr,
                     int nw_stride, u64* __restrict__ mask, int bx_begin, const int32_t* __restrict__ done)
{
    if (done != nullptr && *done != 0) return;
    const int n = *n_ptr;
    const int tile = nms_tri(bx_begin) + (int)blockIdx.x;        // < nms_tri(256) = 32896: exact in float
    int bx = (int)((sqrtf(8.f * (float)tile + 1.f) - 1.f) * 0.5f);
    while (nms_tri(bx + 1) <= tile) ++bx;                        // (the square root may be one off either way)
    while (nms_tri(bx) > tile) --bx;
    const int by = tile - nms_tri(bx);
    if (bx * 64 >= n) return;                                    // (by <= bx: the row chunk exists where the column chunk does)
    __shared__ f32x4 colb[64];
    const int t = threadIdx.x;
    const int jn = bx * 64 + t;
    colb[t] = jn < n ? boxes[jn] : f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    const int i = by * 64 + t;
    if (i >= n) return;
    const f32x4 a = boxes[i];
    u64 bits = 0ull;
    const int jmax = (n - bx * 64) < 64 ? (n - bx * 64) : 64;
    for (int j = 0; j < jmax; ++j) {
        const int jj = bx * 64 + j;
        if (jj > i && iou_gt(a, colb[j], thr)) bits |= 1ull << j;
    }
    mask[(size_t)i * nw_stride + bx] = bits;
}

__device__ __forceinline__ u64 readlane64(u64 v, int lane_uniform)
{
    const int l = __builtin_amdgcn_readfirstlane(lane_uniform);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v & 0xFFFFFFFFull), l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((u64)hi << 32) | lo;
}

// One wave.  removed[] lives in registers: lane l holds words 2 l, 2 l + 1 (capacity 8192 boxes) and 128 + 2 l, 129 + 2 l (16384).  Per
// 64-box chunk c the chunk is resolved serially on a wave-uniform 64-bit "alive" word in SGPRs (s_ff1 + v_readlane per kept box) against
// the diagonal words of its 64 rows, and the kept rows are OR-ed into removed[].
// Round 5 (VERDICT r4 "do this" 6): those row loads used to stand between every two chunks -- chunk c + 1 cannot start before word c + 1 of
// the rows kept in chunk c is known.  On the workload's lists (6000 candidates, 300 kept within the first 15-19 chunks, 10-40 kept boxes per
// chunk) that was one to three round trips per chunk, half of the kernel's 63 us.  Now
//   * word c + 1 travels WITH the diagonal: lane l holds words c, c + 1 of row 64 c + l, fetched two chunks ahead (they depend on
//     nothing); what the boxes kept in chunk c remove from chunk c + 1 comes out of those registers by v_readlane (`fq`);
//   * the kept rows themselves are fetched when the chunk is resolved and consumed TWO chunks later, when the first word the band did
//     not cover is due: a whole chunk's resolution hides their round trip.
// Both go through two LDS slots by LDS-DMA (buffer_load ... lds: no destination registers to keep out of the compiler's way) with a FIXED
// number of DMA instructions per chunk (NMS_DMA = 1 + 24: the band, and 24 row pieces of 1 KB = 24 rows, or 12 rows in two pieces with more
// than 8192 candidates), so that `s_waitcnt vmcnt(NMS_DMA)` is exactly "the slot filled two chunks ago has landed" (vector memory loads
// return in issue order; other loads issued in between only make the wait stronger).  Unused row places fetch row 0: box 0 is always
// kept, OR-ing its row again changes nothing.  A chunk that keeps more boxes than there are places -- the first two or three chunks of a
// list -- waits for the surplus rows at once, sixteen per round trip (what every chunk did before).  The kept set is the same set in the
// same order: only the time at which a bit reaches removed[] changed.
static constexpr int NMS_PIECES = 24;                               // row pieces (1 KB: 16 B per lane) per chunk
static constexpr int NMS_DMA = 1 + NMS_PIECES;                      // DMA instructions per chunk
static constexpr int NMS_SLOT_BYTES = NMS_DMA * 1024;               // 25 KB: [band 1 KB][pieces]
static constexpr int NMS_LDS_BYTES = 2 * NMS_SLOT_BYTES;            // 50 KB of dynamic LDS
typedef __attribute__((address_space(3))) void* nms_lds_ptr;
static_assert(NMS_DMA <= 63, "the look-ahead must fit the 6-bit vmcnt");

// -DNMS_CLOCKS (tools/nms_clocks.py, tools/nms_band.py; timing only, the last four proposals are overwritten): where the kernel's time goes, in 10 ns ticks
#ifdef NMS_CLOCKS
#define NMS_T(k) do { const unsigned long long _t = __builtin_amdgcn_s_memrealtime(); if ((k) != 0 || nms_tl != 0) nms_acc[k] += (float)(_t - nms_tl); nms_tl = _t; } while (0)
#else
#define NMS_T(k) do { } while (0)
#endif

__global__ __launch_bounds__(64)
void nms_reduce_kernel(const u64* __restrict__ mask, int nw_stride, const int32_t* __restrict__ n_ptr,
                       int max_keep, const f32x4* __restrict__ cand_boxes,
                       const int32_t* __restrict__ order,      // optional map to input indices
                       int32_t* __restrict__ keep, f32x4* __restrict__ props,
                       int32_t* __restrict__ n_keep_out,
                       int c_limit,                            // chunks this launch may resolve
                       const int32_t* __restrict__ done_in,    // optional: non-zero = an earlier launch has reduced this list, return at once
                       int32_t* __restrict__ done_out)         // optional: 1 = the outputs are written, 0 = c_limit chunks were not enough (no output)
{
    if (done_in != nullptr && *done_in != 0) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char nms_ring_lds[];               // NMS_LDS_BYTES
    unsigned char* const ring = nms_ring_lds;
    __shared__ int32_t kept_list[2048];
    __shared__ u64 kb_list[256];                 // the kept boxes of every resolved chunk (bit b = box 64 c + b): kept_list is built from them at the end
    const int n = *n_ptr;
    const int lane = threadIdx.x;
    const int nw = (n + 63) >> 6;
    const bool wide = nw > 128;                  // more than 8192 candidates: words 128 .. 255 too
    u64 rem[4] = {0ull, 0ull, 0ull, 0ull};
#ifdef NMS_CLOCKS
    float nms_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long nms_tl = 0;
    const unsigned long long nms_t_in = __builtin_amdgcn_s_memrealtime();
#endif
    int room = max_keep;                         // boxes still to keep
    int c_done = 0;                              // chunks resolved
    u64 fq = 0ull;                               // wave-uniform: what the boxes kept in the previous chunk remove from this one
    // the 16 bytes of a row this lane owns in removed[]: words 2 l, 2 l + 1 and 128 + 2 l, 129 + 2 l (clamped into the row: a lane past
    // the row's end repeats its last words into words of removed[] that do not exist)
    const int wl0 = min(2 * lane, nw_stride - 2), wl1 = min(128 + 2 * lane, nw_stride - 2);

    // (the buffer form of the DMA, as csrc/wino_x3f.hip uses it: rows x nw_stride words = at most 32 MB behind one descriptor)
    const __amdgpu_buffer_rsrc_t mrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<u64*>(mask), 0, 0x7fffffff, 0x00020000);
    auto dma16 = [&](const u64* g, unsigned char* l) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(mrs, (nms_lds_ptr)l, 16, (int)((const unsigned char*)g - (const unsigned char*)mask), 0, 0, 0);
    };
    // a row piece: the row's byte offset is wave-uniform (the instruction's scalar offset), the lane's 16 bytes inside the row a constant
    // register -- 32-bit arithmetic, no branch: a DMA instruction was ~25 instructions of 64-bit pointer arithmetic before, 90 cycles each
    const int row_bytes = nw_stride * 8, vo0 = wl0 * 8, vo1 = wl1 * 8;
    auto dma_piece = [&](int row_index, bool upper, unsigned char* l) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(mrs, (nms_lds_ptr)l, 16, upper ? vo1 : vo0, row_index * row_bytes, 0, 0);
    };
    // band of chunk c -> slot: words c, c + 1 of row 64 c + l.  A row past the last one repeats it (its bit is outside `validm`: nobody
    // reads that lane); a word past the row's end (chunk nw: never used) is the next row's first word -- the mask array is followed by 256
    // bytes of slack for the last row's (proposal_scratch_bytes)
    auto issue_band = [&](int c, unsigned char* slot) {
        const int row = min(c * 64 + lane, n - 1);
        dma16(mask + (size_t)row * nw_stride + min(c, nw_stride - 1), slot);
    };
    auto or16 = [&](const uint4& v, int q0) {
        rem[q0] |= ((u64)v.y << 32) | v.x;
        rem[q0 + 1] |= ((u64)v.w << 32) | v.z;
    };

    if (n > 0) {
        for (int p = 0; p < 2; ++p) {                            // slots of chunks 0, 1: their bands, and row 0 in every row place
            unsigned char* slot = ring + p * NMS_SLOT_BYTES;
            issue_band(p, slot);
#pragma unroll
            // (with `wide` the odd places are row 0's UPPER half, as the main loop's filler: chunks 0 and 1 OR the odd pieces into words
            //  128 .. 255 -- the lower half there made box 0 remove candidate 8192 + j with every box j it removes: ADVICE r5)
            for (int u = 0; u < NMS_PIECES; ++u) dma_piece(0, wide && (u & 1), slot + 1024 + u * 1024);
        }
        // c_limit < nw is phase A of a banded NMS: only the mask's column chunks < c_limit are written, every word >= c_limit of a row holds
        // stale bytes (the storage doubles as the top-N's scratch).  The kept rows are fetched whole, so removed[] carries garbage in its
        // words >= c_limit, and so does `fq` after chunk c_limit - 1 (word c_limit of the band).  Nothing is ever decided from them: a chunk
        // c reads word c of removed[] and the `fq` of chunk c - 1 only, and this loop resolves no chunk >= c_limit; a launch that stops here
        // unfinished writes no output, and the launch that finishes the list starts again from chunk 0 on a complete mask.
        const int c_end = min(nw, c_limit);
        for (int c = 0; c < c_end; ++c) {
            NMS_T(0);
            unsigned char* slot = ring + (c & 1) * NMS_SLOT_BYTES;
            // The slot of this chunk was filled two chunks ago (or above): the previous chunk's NMS_DMA instructions are the only younger ones.
            // The slot is read by ds_read instructions in inline assembly: hipcc puts an s_waitcnt vmcnt(0) in front of every LDS access it
            // can see once an LDS-DMA is in flight (it cannot tell which DMA wrote what), and that wait is the round trip this kernel exists to hide
            const unsigned la = (unsigned)(size_t)slot + 16u * (unsigned)lane;
            uint4 bnd, r0[NMS_PIECES];
            static_assert(NMS_PIECES == 24, "operand lists below");
            asm volatile("s_waitcnt vmcnt(%14)\n\tds_read_b128 %0, %13\n\t"
                         "ds_read_b128 %1, %13 offset:1024\n\tds_read_b128 %2, %13 offset:2048\n\tds_read_b128 %3, %13 offset:3072\n\t"
                         "ds_read_b128 %4, %13 offset:4096\n\tds_read_b128 %5, %13 offset:5120\n\tds_read_b128 %6, %13 offset:6144\n\t"
                         "ds_read_b128 %7, %13 offset:7168\n\tds_read_b128 %8, %13 offset:8192\n\tds_read_b128 %9, %13 offset:9216\n\t"
                         "ds_read_b128 %10, %13 offset:10240\n\tds_read_b128 %11, %13 offset:11264\n\tds_read_b128 %12, %13 offset:12288\n\t"
                         "s_waitcnt lgkmcnt(0)"
                         : "=&v"(bnd), "=&v"(r0[0]), "=&v"(r0[1]), "=&v"(r0[2]), "=&v"(r0[3]), "=&v"(r0[4]), "=&v"(r0[5]), "=&v"(r0[6]), "=&v"(r0[7]),
                           "=&v"(r0[8]), "=&v"(r0[9]), "=&v"(r0[10]), "=&v"(r0[11]) : "v"(la), "n"(NMS_DMA) : "memory");
            asm volatile("ds_read_b128 %0, %12 offset:13312\n\tds_read_b128 %1, %12 offset:14336\n\tds_read_b128 %2, %12 offset:15360\n\t"
                         "ds_read_b128 %3, %12 offset:16384\n\tds_read_b128 %4, %12 offset:17408\n\tds_read_b128 %5, %12 offset:18432\n\t"
                         "ds_read_b128 %6, %12 offset:19456\n\tds_read_b128 %7, %12 offset:20480\n\tds_read_b128 %8, %12 offset:21504\n\t"
                         "ds_read_b128 %9, %12 offset:22528\n\tds_read_b128 %10, %12 offset:23552\n\tds_read_b128 %11, %12 offset:24576\n\t"
                         "s_waitcnt lgkmcnt(0)"
                         : "=&v"(r0[12]), "=&v"(r0[13]), "=&v"(r0[14]), "=&v"(r0[15]), "=&v"(r0[16]), "=&v"(r0[17]), "=&v"(r0[18]), "=&v"(r0[19]),
                           "=&v"(r0[20]), "=&v"(r0[21]), "=&v"(r0[22]), "=&v"(r0[23]) : "v"(la) : "memory");
            NMS_T(1);                                            // [0 -> 1] the wait for the slot and its 25 reads
            const u64 diag = ((u64)bnd.y << 32) | bnd.x, next = ((u64)bnd.w << 32) | bnd.z;
            // the rows kept in chunk c - 2: their words >= c are due now (piece u: row u, or with `wide` row u / 2, half u & 1)
            if (!wide) {
#pragma unroll
                for (int u = 0; u < NMS_PIECES; ++u) or16(r0[u], 0);
            } else {
#pragma unroll
                for (int u = 0; u < NMS_PIECES; ++u) or16(r0[u], 2 * (u & 1));
            }
            const int half = c >> 7, within = c & 127;
            const u64 sel = half == 0 ? ((within & 1) ? rem[1] : rem[0]) : ((within & 1) ? rem[3] : rem[2]);
            const u64 cur = readlane64(sel, within >> 1) | fq;
            const int left = n - c * 64;
            const u64 validm = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
            // The serial part: nothing but the scalar chain per kept box (s_ff1, two v_readlane, three scalar bit operations) -- the list of
            // kept boxes and what they remove from the next chunk are derived from `keepbits` afterwards (this loop was ~35 instructions
            // and an LDS write per kept box, i.e. most of the kernel's time on lists that keep 300 boxes in 15-19 chunks)
            u64 alive = ~cur & validm;
            u64 keepbits = 0ull;
            NMS_T(2);                                            // [1 -> 2] the ORs into removed[], the chunk's word
            while (alive != 0ull) {
                const int b = __ffsll((long long)alive) - 1;
                const u64 bit = 1ull << b;
                keepbits |= bit;
                alive &= ~(readlane64(diag, b) | bit);
            }
            while (__popcll(keepbits) > room) keepbits &= ~(1ull << (63 - __clzll((long long)keepbits)));   // (the list's last chunk: the first `room` of them)
            room -= __popcll(keepbits);
            NMS_T(3);                                            // [2 -> 3] the serial resolution
            if (lane == 0) kb_list[c] = keepbits;
            c_done = c + 1;
            if (room <= 0) break;
            // word c + 1 of the kept rows, OR-ed over the wave: four DPP row rotations, then the four rows of 16 lanes
            {
                const bool mine = (keepbits >> lane) & 1ull;
                unsigned lo = mine ? (unsigned)(next & 0xFFFFFFFFull) : 0u, hi = mine ? (unsigned)(next >> 32) : 0u;
#define NMS_ROR(v, ctl) v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, ctl, 0xf, 0xf, false)
                NMS_ROR(lo, 0x128); NMS_ROR(hi, 0x128); NMS_ROR(lo, 0x124); NMS_ROR(hi, 0x124);
                NMS_ROR(lo, 0x122); NMS_ROR(hi, 0x122); NMS_ROR(lo, 0x121); NMS_ROR(hi, 0x121);
#undef NMS_ROR
                const unsigned glo = (unsigned)__builtin_amdgcn_readlane((int)lo, 0) | (unsigned)__builtin_amdgcn_readlane((int)lo, 16) |
                                     (unsigned)__builtin_amdgcn_readlane((int)lo, 32) | (unsigned)__builtin_amdgcn_readlane((int)lo, 48);
                const unsigned ghi = (unsigned)__builtin_amdgcn_readlane((int)hi, 0) | (unsigned)__builtin_amdgcn_readlane((int)hi, 16) |
                                     (unsigned)__builtin_amdgcn_readlane((int)hi, 32) | (unsigned)__builtin_amdgcn_readlane((int)hi, 48);
                fq = ((u64)ghi << 32) | glo;
            }
            // this chunk's kept rows -> the slot (every read of the slot above has returned); then the band of chunk c + 2.  Always
            // NMS_DMA instructions.
            NMS_T(4);                                            // [3 -> 4] the next chunk's word from the band
            u64 kb = keepbits;
            if (!wide) {
#pragma unroll
                for (int u = 0; u < NMS_PIECES; ++u) {
                    const int ri = kb != 0ull ? c * 64 + __ffsll((long long)kb) - 1 : 0;
                    kb &= kb - 1ull;                             // (0 stays 0)
                    dma_piece(ri, false, slot + 1024 + u * 1024);
                }
            } else {
#pragma unroll
                for (int u = 0; u < NMS_PIECES; u += 2) {
                    const int ri = kb != 0ull ? c * 64 + __ffsll((long long)kb) - 1 : 0;
                    kb &= kb - 1ull;
                    dma_piece(ri, false, slot + 1024 + u * 1024);
                    dma_piece(ri, true, slot + 2048 + u * 1024);
                }
            }
            issue_band(c + 2, slot);
            NMS_T(5);                                            // [4 -> 5] 25 DMA instructions
            // more kept rows than row places (the first chunks of a list: most of the best-scored boxes survive): waited for at once, sixteen
            // rows per round trip
            while (kb != 0ull) {
                constexpr int NB = 16;
                const u64* rows[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    rows[u] = mask;
                    if (kb != 0ull) {
                        const int b = __ffsll((long long)kb) - 1;
                        kb &= kb - 1ull;
                        rows[u] = mask + (size_t)(c * 64 + b) * nw_stride;
                    }
                }
                uint4 v[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) v[u] = *reinterpret_cast<const uint4*>(rows[u] + wl0);
#pragma unroll
                for (int u = 0; u < NB; ++u) or16(v[u], 0);
                if (wide) {
#pragma unroll
                    for (int u = 0; u < NB; ++u) v[u] = *reinterpret_cast<const uint4*>(rows[u] + wl1);
#pragma unroll
                    for (int u = 0; u < NB; ++u) or16(v[u], 2);
                }
            }
            NMS_T(6);                                            // [5 -> 6] the surplus rows
        }
        NMS_T(7);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // (no DMA may still be writing the block's LDS when it ends)
    }
    if (room > 0 && c_done < nw) {                               // unfinished (wave-uniform): the list needs chunks this launch may not resolve
        if (lane == 0 && done_out != nullptr) *done_out = 0;
        return;
    }
    if (lane == 0 && done_out != nullptr) *done_out = 1;
    __syncthreads();
    // kept_list from the chunks' kept bits: lane l expands chunks l, l + 64, ... (its boxes start behind those of all earlier chunks)
    int kept = 0;
    for (int c0 = 0; c0 < c_done; c0 += 64) {
        const int c = c0 + lane;
        int before = kept, total = kept;
        for (int j = c0; j < min(c0 + 64, c_done); ++j) {
            const int cnt = __popcll(kb_list[j]);
            if (j < c) before += cnt;
            total += cnt;
        }
        if (c < c_done) {
            u64 bits = kb_list[c];
            while (bits != 0ull) {
                const int b = __ffsll((long long)bits) - 1;
                bits &= bits - 1ull;
                kept_list[before++] = c * 64 + b;
            }
        }
        kept = total;
    }
    __syncthreads();
    for (int k = lane; k < max_keep; k += 64) {
        if (k < kept) {
            const int ci = kept_list[k];
            if (keep) keep[k] = order ? order[ci] : ci;
            if (props) props[k] = cand_boxes[ci];
        } else {
            if (props) props[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    if (lane == 0) *n_keep_out = kept;
#ifdef NMS_CLOCKS
    if (lane == 0 && props && max_keep >= 4) {
        const unsigned long long t_out = __builtin_amdgcn_s_memrealtime();
        props[max_keep - 1] = f32x4{nms_acc[1], nms_acc[2], nms_acc[3], nms_acc[4]};
        props[max_keep - 2] = f32x4{nms_acc[5], nms_acc[6], (float)(t_out - nms_t_in), (float)c_done};
        props[max_keep - 3] = f32x4{nms_acc[0], nms_acc[7], (float)n, (float)kept};
        props[max_keep - 4] = f32x4{done_in != nullptr ? 1.f : 0.f, (float)c_limit, 0.f, 0.f};      // 1 = written by phase B's reduce: `done` read 0 behind phase A
    }
#endif
}
#undef NMS_T

// ---- host side ------------------------------------------------------------------------------
static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

size_t proposal_scratch_bytes(int a_cap, int pre_cap, int post_cap)
{
    size_t b = 0;
    b += align_up((size_t)a_cap * 8, 256);                       // keys
    b += align_up((size_t)a_cap * 16, 256);                      // boxes_all
    b += align_up((size_t)pre_cap * 16, 256);                    // cand_boxes
    b += align_up((size_t)pre_cap * 4, 256);                     // cand_scores
    b += align_up((size_t)pre_cap * (pre_cap / 64) * 8 + 256, 256);    // mask (+ slack: nms_reduce_kernel's band reads up to 24 B past a row)
    b += align_up((size_t)post_cap * 4, 256);                    // keep
    return b;
}

void proposal_scratch_carve(ProposalScratch& ps, void* base, int a_cap, int pre_cap, int post_cap)
{
    unsigned char* p = static_cast<unsigned char*>(base);
    ps.keys = reinterpret_cast<u64*>(p);         p += align_up((size_t)a_cap * 8, 256);
    ps.boxes_all = reinterpret_cast<float*>(p);  p += align_up((size_t)a_cap * 16, 256);
    ps.cand_boxes = reinterpret_cast<float*>(p); p += align_up((size_t)pre_cap * 16, 256);
    ps.cand_scores = reinterpret_cast<float*>(p); p += align_up((size_t)pre_cap * 4, 256);
    ps.mask = reinterpret_cast<u64*>(p);         p += align_up((size_t)pre_cap * (pre_cap / 64) * 8 + 256, 256);
    ps.keep = reinterpret_cast<int32_t*>(p);
    ps.a_cap = a_cap; ps.pre_cap = pre_cap; ps.post_cap = post_cap;
}

static int pow2_at_least(int v) { int p = 1024; while (p < v) p <<= 1; return p; }

// tmp != NULL (MODE 0): the three-launch form (select -> rank on the whole chip -> emit); tmp holds >= 32 sort_n bytes
template <int MODE>
static int launch_topk(const u64* keys, int n_keys, int K, const float* boxes_src, float ih, float iw,
                       float min_side, int32_t* sorted_idx, float* cand_boxes, float* cand_scores,
                       int32_t* counts, hipStream_t s, void* tmp = nullptr)
{
    const int sort_n = pow2_at_least(K);
    if (sort_n > 16384) return FRCNN_EUNSUPPORTED;
    const size_t lds = (size_t)sort_n * 8 + 4096 * 4 + 64 * 4;
    static const bool no_split = frcnn_knob("FRCNN_TOPK_ONE_BLOCK") != nullptr;          // experiments / A-B tests
    if (MODE == 0 && tmp != nullptr && !no_split) {
        unsigned char* tb = static_cast<unsigned char*>(tmp);
        u64* sel = reinterpret_cast<u64*>(tb);
        f32x4* tboxes = reinterpret_cast<f32x4*>(tb + (size_t)sort_n * 8);
        float* tscores = reinterpret_cast<float*>(tb + (size_t)sort_n * 24);
        int32_t* flags = reinterpret_cast<int32_t*>(tb + (size_t)sort_n * 28);
        auto k1 = topk_sort_kernel<0, true>;
        FRCNN_MAX_LDS_ONCE(k1, 16384 * 8 + 4096 * 4 + 64 * 4);
        hipLaunchKernelGGL(k1, dim3(1), dim3(1024), lds, s, keys, n_keys, K, sort_n, reinterpret_cast<const f32x4*>(boxes_src), ih, iw,
                           min_side, sorted_idx, reinterpret_cast<f32x4*>(cand_boxes), cand_scores, counts, sel);
        int rc = check_launch();
        if (rc) return rc;
        const size_t lds2 = (size_t)sort_n * 8 + 32 * 32 * 4;
        FRCNN_MAX_LDS_ONCE(topk_rank_kernel, 16384 * 8 + 32 * 32 * 4);
        hipLaunchKernelGGL(topk_rank_kernel, dim3(cdiv(K, 32)), dim3(1024), lds2, s, sel, counts, sort_n,
                           reinterpret_cast<const f32x4*>(boxes_src), ih, iw, min_side, sorted_idx, tboxes, tscores, flags);
        rc = check_launch();
        if (rc) return rc;
        hipLaunchKernelGGL(topk_emit_kernel, dim3(1), dim3(1024), 0, s, tboxes, tscores, flags, sort_n, reinterpret_cast<f32x4*>(cand_boxes),
                           cand_scores, counts);
        return check_launch();
    }
    auto kern = topk_sort_kernel<MODE>;
    FRCNN_MAX_LDS_ONCE(kern, 16384 * 8 + 4096 * 4 + 64 * 4);
    hipLaunchKernelGGL(kern, dim3(1), dim3(1024), lds, s, keys, n_keys, K, sort_n,
                       reinterpret_cast<const f32x4*>(boxes_src), ih, iw, min_side, sorted_idx,
                       reinterpret_cast<f32x4*>(cand_boxes), cand_scores, counts, (u64*)nullptr);
    return check_launch();
}

// The NMS of ps.cand_boxes (score-descending, *n_ptr <= 64 nw of them): mask and reduce, in one phase or in two (see NMS_BAND)
static int launch_nms_phases(const ProposalScratch& ps, const int32_t* n_ptr, int nw, bool banded, float thr, int max_keep,
                             const int32_t* order, int32_t* keep, f32x4* props, int32_t* n_keep, hipStream_t s)
{
    const int nw_stride = ps.pre_cap / 64;
    const f32x4* boxes = reinterpret_cast<const f32x4*>(ps.cand_boxes);
    int32_t* done = ps.keep;                     // (nothing else lives there)
    FRCNN_MAX_LDS_ONCE(nms_reduce_kernel, NMS_LDS_BYTES);
    int rc;
    if (!banded) {
        hipLaunchKernelGGL(nms_mask_kernel, dim3(nms_tri(nw)), dim3(64), 0, s, boxes, n_ptr, thr, nw_stride, ps.mask, 0, (const int32_t*)nullptr);
        rc = check_launch();
        if (rc) return rc;
        hipLaunchKernelGGL(nms_reduce_kernel, dim3(1), dim3(64), NMS_LDS_BYTES, s, ps.mask, nw_stride, n_ptr, max_keep, boxes, order, keep,
                           props, n_keep, nw, (const int32_t*)nullptr, (int32_t*)nullptr);
        return check_launch();
    }
    hipLaunchKernelGGL(nms_mask_kernel, dim3(nms_tri(NMS_BAND)), dim3(64), 0, s, boxes, n_ptr, thr, nw_stride, ps.mask, 0, (const int32_t*)nullptr);
    rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(nms_reduce_kernel, dim3(1), dim3(64), NMS_LDS_BYTES, s, ps.mask, nw_stride, n_ptr, max_keep, boxes, order, keep,
                       props, n_keep, NMS_BAND, (const int32_t*)nullptr, done);
    rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(nms_mask_kernel, dim3(nms_tri(nw) - nms_tri(NMS_BAND)), dim3(64), 0, s, boxes, n_ptr, thr, nw_stride, ps.mask, NMS_BAND,
                       (const int32_t*)done);
    rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(nms_reduce_kernel, dim3(1), dim3(64), NMS_LDS_BYTES, s, ps.mask, nw_stride, n_ptr, max_keep, boxes, order, keep,
                       props, n_keep, nw, (const int32_t*)done, done);
    return check_launch();
}

int launch_rpn_proposals(const ProposalScratch& ps, const float* head, int ld_head,
                         const float* anchor_map, const float* valid_map, int fh, int fw,
                         int image_h, int image_w, int pre_nms, int post_nms, float nms_thr,
                         float min_side, float* scores, int32_t* sorted_idx, float* props,
                         int32_t* counts, hipStream_t s)
{
    const int A = fh * fw * 9;
    if (A < 1 || A > ps.a_cap || pre_nms < 1 || pre_nms > ps.pre_cap || post_nms < 1 ||
        post_nms > ps.post_cap || post_nms > 2048 || ld_head < 45)
        return FRCNN_EINVAL;
    hipLaunchKernelGGL(rpn_decode_kernel, dim3(cdiv(A, 256)), dim3(256), 0, s, head, ld_head, anchor_map,
                       valid_map, A, scores, reinterpret_cast<f32x4*>(ps.boxes_all), ps.keys);
    int rc = check_launch();
    if (rc) return rc;
    // (the NMS bit matrix is written after the top-N: its storage doubles as the top-N's scratch)
    rc = launch_topk<0>(ps.keys, A, pre_nms, ps.boxes_all, (float)image_h, (float)image_w, min_side,
                        sorted_idx, ps.cand_boxes, ps.cand_scores, counts, s, ps.mask);
    if (rc) return rc;
    // post_nms is small against pre_nms in every use of the RPN: banded wherever there is anything behind the band
    return launch_nms_phases(ps, counts + 1, cdiv(pre_nms, 64), cdiv(pre_nms, 64) > NMS_BAND, nms_thr, post_nms, nullptr, nullptr,
                             reinterpret_cast<f32x4*>(props), counts + 2, s);
}

int launch_nms(const ProposalScratch& ps, const float* boxes, const float* scores, int n, float thr,
               int max_keep, int32_t* keep, int32_t* n_keep, hipStream_t s)
{
    if (n < 0 || n > ps.pre_cap || n > ps.a_cap || max_keep < 1 || max_keep > 2048) return FRCNN_EINVAL;
    if (n == 0) {
        FRCNN_HIP_TRY(hipMemsetAsync(n_keep, 0, sizeof(int32_t), s));
        return FRCNN_OK;
    }
    hipLaunchKernelGGL(nms_keys_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, scores, n, ps.keys);
    int rc = check_launch();
    if (rc) return rc;
    // sorted order -> ps.keep is too small for n indices; reuse boxes_all's tail as int scratch
    int32_t* order = reinterpret_cast<int32_t*>(ps.boxes_all);
    int32_t* counts = order + ps.a_cap;          // boxes_all holds 4*a_cap floats; use [a_cap, a_cap+4)
    rc = launch_topk<1>(ps.keys, n, n, boxes, 0.f, 0.f, 0.f, order, ps.cand_boxes, ps.cand_scores, counts, s);
    if (rc) return rc;
    // Two phases only where they can pay.  The band was measured on lists that keep a box in four of their best-scored candidates (300
    // within 19 chunks of 64), with a margin of 1.5: a caller that wants more than a quarter of the band's 64 NMS_BAND boxes is likely
    // to need phase B, and then pays phase A's reduce twice.  And what the band saves must outweigh phase B's two empty launches (a few
    // microseconds, about a thousand tiles of the mask): at least as many column chunks behind the band as in it, i.e. under a quarter
    // of the tiles in phase A.  Every other call is one mask over the triangle and one reduce.
    const int nw = cdiv(n, 64);
    const bool banded = nw >= 2 * NMS_BAND && 4 * max_keep <= 64 * NMS_BAND;
    return launch_nms_phases(ps, counts + 1, nw, banded, thr, max_keep, order, keep, nullptr, n_keep, s);
}

}  // namespace frcnn

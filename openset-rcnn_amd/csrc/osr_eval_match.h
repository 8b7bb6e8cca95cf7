// What the evaluators' match kernels share: one clamped segment read, one group list (compaction and stable rank), one threshold /
// area-range table, one greedy pass of a wave and one packing of its results into the flag words. Users:
//   osr_coco_eval.hip        cm_match_kernel   everything
//   osr_os_coco_eval.hip     om_match_kernel   everything
//   osr_lvis_eval.hip        lv_group_kernel   the compaction and the rank count (an image's rows, cut across its categories)
//                            lv_match_kernel   the segment read, the tables, the greedy pass and the flag packer at 512 detections a group
//   osr_voc_eval.hip         vm_match_kernel   the segment read, the compaction and the rank count
//   osr_proposal_recall.hip  pr_recall_kernel  the segment read (its limits are its own PR_*: its LDS plan takes 2048 rows, 1024 ground truths)
// Each of these is a place where a one-sided change would break bit-exactness against numpy: the stable tie order, the
// min(t, 1 - 1e-10) threshold, the clamped read, the 2-bit results. What a kernel keeps for itself is what differs for a reason:
//   - its similarity function. cm_bbox_sim takes fp32 differences and widens them, om_bbox_sim widens first and divides by
//     fmax(uni, 1e-300): each rounds like its own numpy specification;
//   - what a group and its ground-truth sets are, the set bits of g_meta, and how the similarity matrix is indexed (by rank / by row);
//   - VOC's argmax / first-rank scheme and proposal recall's rounds, which are other algorithms.
#pragma once
#include <type_traits>

#include "osr_common.h"

#define EM_THREADS 1024
#define EM_WAVES (EM_THREADS / 64)
#define EM_MAX_CAP 1024
#define EM_MAX_DET 128
#define EM_MAX_T 16
#define EM_MAX_A 8
#define EM_MAX_G 4096

// ---- segment k of an offset table, clamped: a table that lies cannot send a read past num_gt or a loop past the call's maximum ----
__device__ __forceinline__ void em_segment(const int32_t* __restrict__ off, int k, int num_gt, int max_len, int* g0, int* G) {
    const int a = min(max(off[k], 0), num_gt);
    *G = min(max(off[k + 1] - off[k], 0), min(num_gt - a, max_len));
    *g0 = a;
}

// ---- the group's list: its rows in row order. pick(r, &key) says whether row r < cnt is a member and gives its key; it is called once
// per row, must hold no barrier and may have side effects. Called by the whole block (cnt is uniform: the scans' barriers are too);
// -> the number of members. The lists are complete after the caller's next barrier. ----
template <class Key, class Pick>
__device__ __forceinline__ int em_compact(int cnt, int* scan, int* c_row, Key* c_key, Pick pick) {
    int D = 0;
    for (int base = 0; base < cnt; base += EM_THREADS) {
        const int r = base + threadIdx.x;
        Key key = 0;
        const bool mine = r < cnt && pick(r, &key);
        int total;
        const int pos = osr_block_excl_scan(mine ? 1 : 0, scan, &total);
        if (mine) c_row[D + pos] = r, c_key[D + pos] = key;
        D += total;
    }
    return D;
}

// the members that precede member m: a higher key, or the same key and a lower row (mergesort's stable descending order)
template <class Key>
__device__ __forceinline__ int em_stable_before(const Key* c_key, int D, int m) {
    const Key key = c_key[m];
    int before = 0;
    for (int o = 0; o < D; ++o) before += (c_key[o] > key) || (c_key[o] == key && o < m);
    return before;
}

// ---- thresholds and area ranges of the COCO-style kernels ----
struct EmTables {
    double thr[EM_MAX_T];      // min(t, 1 - 1e-10), formed on the host in fp64; padded with 2.0 (no similarity reaches it)
    double rng[EM_MAX_A * 2];  // (lo, hi) per area range; padded with 0
};

static inline void em_fill_tables(EmTables* tb, const double* iou_thrs, int num_thrs, const double* area_rng, int num_areas) {
    for (int t = 0; t < EM_MAX_T; ++t) tb->thr[t] = t < num_thrs ? (iou_thrs[t] < 1 - 1e-10 ? iou_thrs[t] : 1 - 1e-10) : 2.0;
    for (int a = 0; a < EM_MAX_A * 2; ++a) tb->rng[a] = a < num_areas * 2 ? area_rng[a] : 0.0;
}

// rows outside every list read 0 / -1 / -1: flags, rank and (if asked for) match are preset on the kernel's stream
static inline bool em_preset(uint32_t* flags, int64_t flag_words, int32_t* rank, int64_t rows, int32_t* match, int64_t match_words, hipStream_t st) {
    return hipMemsetAsync(flags, 0, (size_t)flag_words * 4, st) == hipSuccess && hipMemsetAsync(rank, 0xff, (size_t)rows * 4, st) == hipSuccess &&
           (!match || hipMemsetAsync(match, 0xff, (size_t)match_words * 4, st) == hipSuccess);
}

// ---- g_meta, one uint16 per ground truth: bit a = "ignored in area range a", bit 8 = crowd, bits 9-10 = the caller's set ----
#define EM_CROWD 0x100
#define EM_SET_SHIFT 9

__device__ __forceinline__ int em_ignored_bits(bool always_ignored, double area, const double* rng, int A) {
    int m = 0;
    for (int a = 0; a < A; ++a) m |= (always_ignored || area < rng[a * 2] || area > rng[a * 2 + 1]) ? 1 << a : 0;
    return m;
}

// ---- one wave, one (set, area range, threshold) chain ----
// The larger similarity wins; equal similarities go to the higher key and equal keys to the higher position; j < 0: no candidate.
// Without a key the position is the key, and two values travel instead of three. The test stays ONE short-circuit expression: with the
// tie test formed ahead of it the compiler branched twice more per step, 1 % of osr_coco_match's launch.
template <bool KEYED>
__device__ __forceinline__ void em_wave_best(double& s, int& k, int& j) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const double os = __shfl_xor(s, d, 64);
        const int oj = __shfl_xor(j, d, 64), ok = KEYED ? __shfl_xor(k, d, 64) : 0;
        if (oj >= 0 && (j < 0 || os > s || (os == s && (KEYED ? ok > k || (ok == k && oj > j) : oj > j)))) s = os, k = ok, j = oj;
    }
}

// The pass walks its M detections in rank order. Per detection the lanes stride over the G ground truths (lane l owns j = l, l + 64, ..:
// its "matched" bits are ONE 64-bit register, G <= 4096), skip those outside `set` (set < 0: there are no sets), keep the best available
// candidate among the not-ignored and among the ignored ones, and one wave reduction picks the winner. A crowd never retires; an
// unmatched detection outside the area range is ignored. row(d): detection d's row of similarities; key_of(j): the tie key of ground
// truth j (KEYED only); a match g0 + j goes to match0[d_row[d] * match_stride] (match0 null: nowhere). -> the lane's results, two bits
// per detection (bit 0 matched, bit 1 ignored): bits 0-1 detection `lane`, bits 2-3 detection 64 + `lane`, and so on.
// MAX_DET is the most detections a group of the kernel lists. It sizes the word a lane's results are KEPT in (em_res_t: a byte holds
// two detections, which is EM_MAX_DET = 128 and what the COCO and open-set kernels use; LVIS lists up to 512); the pass itself
// gathers them in one 32-bit register whatever MAX_DET is.
template <int MAX_DET>
struct EmRes {
    static_assert(MAX_DET >= 64 && MAX_DET <= 1024 && MAX_DET % 64 == 0, "a lane's results are at most one 32-bit register: 16 detections");
    typedef std::conditional_t<MAX_DET <= 128, uint8_t, std::conditional_t<MAX_DET <= 512, uint16_t, uint32_t>> type;
};
template <int MAX_DET>
using em_res_t = typename EmRes<MAX_DET>::type;
static_assert(sizeof(em_res_t<EM_MAX_DET>) == 1, "a lane's result byte holds two detections");
static_assert(EM_MAX_G <= 64 * 64, "a lane's matched bits are one 64-bit register");

template <bool KEYED, int MAX_DET = EM_MAX_DET, class Row, class KeyOf>
__device__ __forceinline__ uint32_t em_greedy_pass(const uint16_t* g_meta, int G, int set, double thr, int a, double lo, double hi, const double* d_area,
                                                   const int* d_row, int M, Row row, KeyOf key_of, int32_t* match0, int64_t match_stride, int g0) {
    static_assert(sizeof(em_res_t<MAX_DET>) * 256 >= MAX_DET, "the caller's result word holds two bits for each of a lane's MAX_DET / 64 detections");
    const int lane = threadIdx.x & 63, steps = (G + 63) >> 6;
    unsigned long long taken = 0;  // bit q: ground truth q * 64 + lane is matched in this pass
    uint32_t acc = 0;
    for (int d = 0; d < M; ++d) {
        const double* Sd = row(d);
        double sn = 0.0, si = 0.0;
        int jn = -1, ji = -1, kn = -1, ki = -1;
        for (int q = 0; q < steps; ++q) {
            const int j = (q << 6) + lane;
            if (j >= G) break;
            const int m = g_meta[j];
            if (set >= 0 && ((m >> EM_SET_SHIFT) & 3) != set) continue;
            if (((taken >> q) & 1) && !(m & EM_CROWD)) continue;
            const double sv = Sd[j];
            if (!(sv >= thr)) continue;  // (a NaN is skipped as well)
            const int key = KEYED ? key_of(j) : j;
            // without a key j ascends, so `>=` is "larger, or equal and the higher position"
            if ((m >> a) & 1) {
                if (ji < 0 || (KEYED ? sv > si || (sv == si && key > ki) : sv >= si)) si = sv, ji = j, ki = key;
            } else {
                if (jn < 0 || (KEYED ? sv > sn || (sv == sn && key > kn) : sv >= sn)) sn = sv, jn = j, kn = key;
            }
        }
        em_wave_best<KEYED>(sn, kn, jn);
        if (jn < 0) {
            em_wave_best<KEYED>(si, ki, ji);
            jn = ji;
        }
        uint32_t out;
        if (jn >= 0) {
            if ((jn & 63) == lane) taken |= 1ull << (jn >> 6);
            out = 1u | (uint32_t)((g_meta[jn] >> a) & 1) << 1;
        } else {
            out = (d_area[d] < lo || d_area[d] > hi) ? 2u : 0u;
        }
        if ((d & 63) == lane) acc |= out << ((d >> 6) * 2);
        if (lane == 0 && match0 && jn >= 0) match0[d_row[d] * match_stride] = g0 + jn;
    }
    return acc;
}

// the flag word of detection d from the T passes first_pass .. first_pass + T - 1 of res[pass][lane]: bit t matched, bit 16 + t ignored
template <int MAX_DET = EM_MAX_DET>
__device__ __forceinline__ uint32_t em_flag_word(const em_res_t<MAX_DET> (*res)[64], int first_pass, int T, int d) {
    uint32_t w = 0;
    for (int t = 0; t < T; ++t) {
        const uint32_t b = res[first_pass + t][d & 63] >> ((d >> 6) * 2);
        w |= (b & 1u) << t | ((b >> 1) & 1u) << (16 + t);
    }
    return w;
}

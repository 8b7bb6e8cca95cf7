// The pixel passes of the segmentation evaluators for gfx950 (include/osr.h: osr_semseg_confusion, osr_panoptic_pair_counts,
// osr_pq_accumulate). All three count with integer atomics only, so a repeat gives the same bits; nothing syncs with the host.
//
// The two pixel kernels share one shape. The grid is sized by the CUs, not by the pixels: a workgroup owns a contiguous chunk of the
// image and thread t walks the pixels t, t + 256, .. of it. A thread keeps ONE open run (bin, count): while the bin of its next pixel
// equals the open one it only counts, and it adds the run to the histogram when the bin changes. On blocky maps a thread then adds a
// few times per chunk, and the constant map does not hammer one LDS address. The histogram lives in LDS when it fits (int32, flushed
// with one 64-bit / 32-bit integer atomic per non-zero bin and workgroup); when it does not (C > 126, or a large G x P table) the
// runs go straight to global memory with integer atomics.
//
// osr_pq_accumulate is ONE workgroup of 1024 threads per image:
//   1. per predicted id: its area (column sum, VOID and unlisted rows included), its slot, the row of its slot's crowd_pick;
//   2. every (g, p) pair in parallel: the match test, marks for both sides, per row the number of matches and the lowest matching p;
//   3. one thread per category slot walks its rows in ascending g and adds the matches' IoU onto the running sum in ascending p: the
//      (g, p) order of the contract. A row with one match (the only case with consistent areas) costs one load; a row with several
//      is walked in full;
//   4. fn per unmatched non-crowd row, fp per unmatched predicted id that VOID and the crowd do not cover by more than half.
#include "osr_common.h"

#define SE_THREADS 256
#define SE_LDS_MAX_C 126                      // (C + 1)^2 int32 <= 64 KB
#define PP_MAX_G 1023
#define PP_MAX_P 2047
#define PQ_THREADS 1024

static int se_cu_count() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    return cus;
}

// chunk: pixels per workgroup, a multiple of SE_THREADS * 4; *blocks receives ceil(hw / chunk) <= max_blocks
static int64_t se_chunk(int64_t hw, int max_blocks, int* blocks) {
    const int64_t unit = SE_THREADS * 4;
    int64_t chunk = ((hw + max_blocks - 1) / max_blocks + unit - 1) / unit * unit;
    *blocks = (int)((hw + chunk - 1) / chunk);
    return chunk;
}

__device__ __forceinline__ void se_add64(int64_t* p, long long v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }

__device__ __forceinline__ void se_wave_count(int v, int64_t* dst) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0 && v) se_add64(dst, v);
}

// ---- osr_semseg_confusion -----------------------------------------------------------------------------------------------------------
struct SeRun {
    int bin, n;
};

// lds_bins > 0: the histogram is hist[lds_bins] in LDS; 0: conf itself
__device__ __forceinline__ void se_conf_close(const SeRun& r, int* hist, int lds_bins, int64_t* conf) {
    if (r.n == 0) return;
    if (lds_bins) atomicAdd(hist + r.bin, r.n);
    else se_add64(conf + r.bin, r.n);
}

__device__ __forceinline__ void se_conf_pixel(int pred, int gt, int C, int ignore_value, SeRun& run, int& invalid, int* hist, int lds_bins, int64_t* conf) {
    const bool ignored = gt == ignore_value;
    const int col = ignored ? C : gt;
    if ((!ignored && gt >= C) || pred < 0 || pred >= C) {
        ++invalid;
        return;
    }
    const int bin = pred * (C + 1) + col;
    if (bin == run.bin) {
        ++run.n;
    } else {
        se_conf_close(run, hist, lds_bins, conf);
        run.bin = bin, run.n = 1;
    }
}

// strict comparisons from class 0 up: the lowest class wins a tie, NaN never replaces the incumbent (osr_semseg_resample's rule)
template <int V>
__device__ __forceinline__ void se_argmax(const float* __restrict__ values, int64_t hw, int64_t p, int C, int* arg) {
    float best[V];
#pragma unroll
    for (int v = 0; v < V; ++v) best[v] = 0.f, arg[v] = 0;
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
        float e[V];
        if constexpr (V == 4) {
            const float4 q = *reinterpret_cast<const float4*>(values + (int64_t)c * hw + p);
            e[0] = q.x, e[1] = q.y, e[2] = q.z, e[3] = q.w;
        } else {
            e[0] = values[(int64_t)c * hw + p];
        }
#pragma unroll
        for (int v = 0; v < V; ++v)
            if (c == 0 || e[v] > best[v]) best[v] = e[v], arg[v] = c;
    }
}

// V pixels per thread and step (V == 4: hw a multiple of 4, pred / values 16-byte and gt 4-byte aligned)
template <bool VALUES, int V>
__global__ __launch_bounds__(SE_THREADS) void se_confusion_kernel(const void* __restrict__ pred, const uint8_t* __restrict__ gt, int64_t hw, int64_t chunk,
                                                                 int C, int ignore_value, int lds_bins, int64_t* __restrict__ conf,
                                                                 int64_t* __restrict__ invalid) {
    extern __shared__ __align__(16) int se_hist[];
    for (int i = threadIdx.x; i < lds_bins; i += SE_THREADS) se_hist[i] = 0;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = min(lo + chunk, hw);
    SeRun run = {-1, 0};
    int bad = 0;
    for (int64_t p = lo + (int64_t)threadIdx.x * V; p < hi; p += SE_THREADS * V) {  // (V == 4: p + 3 < hw, since hw and lo are multiples of 4)
        int lab[V], g[V];
        if constexpr (VALUES) {
            se_argmax<V>((const float*)pred, hw, p, C, lab);
        } else if constexpr (V == 4) {
            const int4 q = *reinterpret_cast<const int4*>((const int32_t*)pred + p);
            lab[0] = q.x, lab[1] = q.y, lab[2] = q.z, lab[3] = q.w;
        } else {
            lab[0] = ((const int32_t*)pred)[p];
        }
        if constexpr (V == 4) {
            const uchar4 q = *reinterpret_cast<const uchar4*>(gt + p);
            g[0] = q.x, g[1] = q.y, g[2] = q.z, g[3] = q.w;
        } else {
            g[0] = gt[p];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) se_conf_pixel(lab[v], g[v], C, ignore_value, run, bad, se_hist, lds_bins, conf);
    }
    se_conf_close(run, se_hist, lds_bins, conf);
    se_wave_count(bad, invalid);
    if (lds_bins) {
        __syncthreads();
        for (int i = threadIdx.x; i < lds_bins; i += SE_THREADS) {
            const int n = se_hist[i];
            if (n) se_add64(conf + i, n);
        }
    }
}

static bool se_shape_ok(int32_t h, int32_t w) { return h >= 1 && w >= 1 && (int64_t)h * w <= (1LL << 30); }

extern "C" osr_status osr_semseg_confusion(const void* pred, int32_t mode, const uint8_t* gt, int32_t h, int32_t w, int32_t num_classes,
                                           int32_t ignore_value, int64_t* conf, int64_t* invalid, void* stream) {
    OSR_REQUIRE(pred && gt && conf && invalid, OSR_ERR_INVALID_ARG, "osr_semseg_confusion: null pointer");
    OSR_REQUIRE(mode == OSR_CONF_LABELS || mode == OSR_CONF_VALUES, OSR_ERR_INVALID_ARG, "osr_semseg_confusion: mode %d", mode);
    OSR_REQUIRE(num_classes >= 1 && num_classes <= 255, OSR_ERR_INVALID_ARG, "osr_semseg_confusion: 1 .. 255 classes, got %d", num_classes);
    OSR_REQUIRE(se_shape_ok(h, w), OSR_ERR_INVALID_ARG, "osr_semseg_confusion: map %d x %d", h, w);
    OSR_REQUIRE(((uintptr_t)pred & 3) == 0 && ((uintptr_t)conf & 7) == 0 && ((uintptr_t)invalid & 7) == 0, OSR_ERR_INVALID_ARG,
                "osr_semseg_confusion: misaligned pointer");
    const int64_t hw = (int64_t)h * w;
    const int C = num_classes, bins = (C + 1) * (C + 1);
    const int lds_bins = C <= SE_LDS_MAX_C ? bins : 0;
    // a 64 KB histogram leaves room for two workgroups per CU; the small ones for four
    int blocks;
    const int64_t chunk = se_chunk(hw, se_cu_count() * (lds_bins * 4 > 32768 ? 2 : 4), &blocks);
    const bool vec = hw % 4 == 0 && ((uintptr_t)pred & 15) == 0 && ((uintptr_t)gt & 3) == 0;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)lds_bins * 4;
#define SE_LAUNCH(VALUES, V) \
    hipLaunchKernelGGL((se_confusion_kernel<VALUES, V>), dim3(blocks), dim3(SE_THREADS), lds, st, pred, gt, hw, chunk, C, ignore_value, lds_bins, conf, invalid)
    if (mode == OSR_CONF_VALUES) {
        if (vec) SE_LAUNCH(true, 4);
        else SE_LAUNCH(true, 1);
    } else {
        if (vec) SE_LAUNCH(false, 4);
        else SE_LAUNCH(false, 1);
    }
#undef SE_LAUNCH
    OSR_CHECK_LAUNCH("osr_semseg_confusion");
    return OSR_OK;
}

// ---- osr_panoptic_pair_counts -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pp_close(const SeRun& r, int* hist, int lds_bins, int32_t* counts) {
    if (r.n == 0) return;
    atomicAdd(lds_bins ? hist + r.bin : counts + r.bin, r.n);
}

// row of a ground-truth id: 0 for VOID, 1 + i for ids[i], G + 1 for an id that is not listed (ids strictly ascending)
__device__ __forceinline__ int pp_row(const int* ids, int G, int id) {
    if (id == 0) return 0;
    int lo = 0, hi = G;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ids[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return (lo < G && ids[lo] == id) ? 1 + lo : G + 1;
}

__global__ __launch_bounds__(SE_THREADS) void pp_pair_counts_kernel(const uint8_t* __restrict__ rgb, const int32_t* __restrict__ gt_ids, int G,
                                                                   const int32_t* __restrict__ pred, int P, int64_t hw, int64_t chunk, int lds_bins,
                                                                   int32_t* __restrict__ counts, int64_t* __restrict__ flags) {
    __shared__ int ids[PP_MAX_G + 1];
    extern __shared__ __align__(16) int se_hist[];
    for (int i = threadIdx.x; i < G; i += SE_THREADS) ids[i] = gt_ids[i];
    for (int i = threadIdx.x; i < lds_bins; i += SE_THREADS) se_hist[i] = 0;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = min(lo + chunk, hw);
    SeRun run = {-1, 0};
    int bad = 0, last_id = 0, last_row = 0;  // the search runs once per run of equal ids
    for (int64_t p = lo + threadIdx.x; p < hi; p += SE_THREADS) {
        const uint8_t* px = rgb + p * 3;
        const int id = (int)px[0] | ((int)px[1] << 8) | ((int)px[2] << 16);
        const int q = pred[p];
        if (id != last_id) last_id = id, last_row = pp_row(ids, G, id);
        if (q < 0 || q > P) {
            ++bad;
            continue;
        }
        const int bin = last_row * (P + 1) + q;
        if (bin == run.bin) {
            ++run.n;
        } else {
            pp_close(run, se_hist, lds_bins, counts);
            run.bin = bin, run.n = 1;
        }
    }
    pp_close(run, se_hist, lds_bins, counts);
    se_wave_count(bad, flags);
    if (lds_bins) {
        __syncthreads();
        for (int i = threadIdx.x; i < lds_bins; i += SE_THREADS) {
            const int n = se_hist[i];
            if (n) atomicAdd(counts + i, n);
        }
    }
}

static osr_status pp_limits(const char* name, int32_t G, int32_t P) {
    OSR_REQUIRE(G >= 0 && P >= 0, OSR_ERR_INVALID_ARG, "%s: G %d, P %d", name, G, P);
    OSR_REQUIRE(G <= PP_MAX_G && P <= PP_MAX_P, OSR_ERR_UNSUPPORTED, "%s: at most %d ground-truth and %d predicted segments per image, got %d and %d", name,
                PP_MAX_G, PP_MAX_P, G, P);
    return OSR_OK;
}

extern "C" osr_status osr_panoptic_pair_counts(const uint8_t* gt_rgb, const int32_t* gt_ids, int32_t num_gt, const int32_t* pred, int32_t num_pred,
                                               int32_t h, int32_t w, int32_t* counts, int64_t* flags, void* stream) {
    const osr_status lim = pp_limits("osr_panoptic_pair_counts", num_gt, num_pred);
    if (lim != OSR_OK) return lim;
    OSR_REQUIRE(gt_rgb && pred && counts && flags && (num_gt == 0 || gt_ids), OSR_ERR_INVALID_ARG, "osr_panoptic_pair_counts: null pointer");
    OSR_REQUIRE(se_shape_ok(h, w), OSR_ERR_INVALID_ARG, "osr_panoptic_pair_counts: map %d x %d", h, w);
    OSR_REQUIRE(((uintptr_t)pred & 3) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)flags & 7) == 0 && ((uintptr_t)gt_ids & 3) == 0,
                OSR_ERR_INVALID_ARG, "osr_panoptic_pair_counts: misaligned pointer");
    const int64_t hw = (int64_t)h * w, bins = (int64_t)(num_gt + 2) * (num_pred + 1);
    const int lds_bins = bins <= 12 * 1024 ? (int)bins : 0;  // 48 KB beside the 4 KB id table
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)bins * 4, st) != hipSuccess) {
        osr_set_error("osr_panoptic_pair_counts: hipMemsetAsync failed");
        return OSR_ERR_LAUNCH;
    }
    int blocks;
    const int64_t chunk = se_chunk(hw, se_cu_count() * (lds_bins * 4 > 24576 ? 2 : 4), &blocks);
    hipLaunchKernelGGL(pp_pair_counts_kernel, dim3(blocks), dim3(SE_THREADS), (size_t)lds_bins * 4, st, gt_rgb, gt_ids, num_gt, pred, num_pred, hw, chunk,
                       lds_bins, counts, flags);
    OSR_CHECK_LAUNCH("osr_panoptic_pair_counts");
    return OSR_OK;
}

// ---- osr_pq_accumulate --------------------------------------------------------------------------------------------------------------
// the one place the match test is written: phases 2 and 3 must agree bit for bit
__device__ __forceinline__ bool pq_match(int inter, int area_p, int area_g, int void_p, double* iou) {
    const long long uni = (long long)area_p + area_g - inter - void_p;
    *iou = (double)inter / (double)uni;
    return *iou > 0.5;
}

__global__ __launch_bounds__(PQ_THREADS) void pq_accumulate_kernel(const int32_t* __restrict__ counts, int G, int P, const int32_t* __restrict__ gt_meta,
                                                                   const int32_t* __restrict__ pred_slot, int ncat, int64_t* __restrict__ pq_counts,
                                                                   double* __restrict__ pq_iou, int64_t* __restrict__ flags) {
    __shared__ int p_area[PP_MAX_P + 1], p_slot[PP_MAX_P + 1], p_matched[PP_MAX_P + 1], p_crowd_row[PP_MAX_P + 1];  // index: predicted id (0 unused)
    __shared__ int g_slot[PP_MAX_G + 1], g_kind[PP_MAX_G + 1], g_area[PP_MAX_G + 1], g_matched[PP_MAX_G + 1], g_nmatch[PP_MAX_G + 1], g_first[PP_MAX_G + 1];
    const int tid = threadIdx.x, pitch = P + 1;
    int bad_slot = 0, empty = 0;
    // g_kind: bit 0 crowd, bit 1 crowd_pick, bit 2 slot outside [0, ncat) (the row then takes part in nothing but the areas)
    for (int g = tid; g < G; g += PQ_THREADS) {
        const int slot = gt_meta[g * 4 + 0];
        const bool ok = slot >= 0 && slot < ncat;
        g_slot[g] = slot;
        g_kind[g] = (gt_meta[g * 4 + 1] ? 1 : 0) | (gt_meta[g * 4 + 3] ? 2 : 0) | (ok ? 0 : 4);
        g_area[g] = gt_meta[g * 4 + 2];
        g_matched[g] = 0, g_nmatch[g] = 0, g_first[g] = 0x7fffffff;
        if (!ok) ++bad_slot;
    }
    __syncthreads();
    // 1. the predicted ids
    for (int p = 1 + tid; p <= P; p += PQ_THREADS) {
        int area = 0;
        for (int r = 0; r < G + 2; ++r) area += counts[(int64_t)r * pitch + p];
        const int slot = pred_slot[p - 1];
        int crow = -1;
        for (int g = 0; g < G; ++g)
            if ((g_kind[g] & 6) == 2 && g_slot[g] == slot) crow = g;  // (the contract marks one row per slot)
        p_area[p] = area, p_slot[p] = slot, p_matched[p] = 0, p_crowd_row[p] = crow;
        if (slot < 0 || slot >= ncat) ++bad_slot;
        else if (area == 0) ++empty;
    }
    __syncthreads();
    // 2. every pair
    const int64_t pairs = (int64_t)G * P;
    for (int64_t i = tid; i < pairs; i += PQ_THREADS) {
        const int g = (int)(i / P), p = (int)(i % P) + 1;
        if (g_kind[g] & 5) continue;
        const int inter = counts[(int64_t)(1 + g) * pitch + p];
        if (inter <= 0 || p_slot[p] != g_slot[g]) continue;
        double iou;
        if (!pq_match(inter, p_area[p], g_area[g], counts[p], &iou)) continue;
        g_matched[g] = 1, p_matched[p] = 1;  // (every writer writes 1)
        atomicAdd(g_nmatch + g, 1);
        atomicMin(g_first + g, p);
    }
    __syncthreads();
    // 3. one thread per slot, ascending (g, p)
    for (int s = tid; s < ncat; s += PQ_THREADS) {
        double sum = pq_iou[s];
        long long tp = 0;
        for (int g = 0; g < G; ++g) {
            if (g_nmatch[g] == 0 || g_slot[g] != s) continue;
            const int p0 = g_first[g], p1 = g_nmatch[g] == 1 ? p0 : P;
            for (int p = p0; p <= p1; ++p) {
                const int inter = counts[(int64_t)(1 + g) * pitch + p];
                if (inter <= 0 || p_slot[p] != s) continue;
                double iou;
                if (pq_match(inter, p_area[p], g_area[g], counts[p], &iou)) sum += iou, ++tp;
            }
        }
        if (tp) {
            pq_iou[s] = sum;
            pq_counts[(int64_t)s * 3 + 0] += tp;  // (this thread owns the slot's tp; fp and fn below are other addresses)
        }
    }
    // 4. what is left over
    for (int g = tid; g < G; g += PQ_THREADS)
        if ((g_kind[g] & 5) == 0 && !g_matched[g]) se_add64(pq_counts + (int64_t)g_slot[g] * 3 + 2, 1);
    for (int p = 1 + tid; p <= P; p += PQ_THREADS) {
        const int slot = p_slot[p], area = p_area[p];
        if (p_matched[p] || slot < 0 || slot >= ncat || area == 0) continue;
        const int crow = p_crowd_row[p];
        const long long covered = (long long)counts[p] + (crow >= 0 ? counts[(int64_t)(1 + crow) * pitch + p] : 0);
        if ((double)covered / (double)area > 0.5) continue;
        se_add64(pq_counts + (int64_t)slot * 3 + 1, 1);
    }
    if (empty) se_add64(flags + 1, empty);
    if (bad_slot) se_add64(flags + 2, bad_slot);
}

extern "C" osr_status osr_pq_accumulate(const int32_t* counts, int32_t num_gt, int32_t num_pred, const int32_t* gt_meta, const int32_t* pred_slot,
                                        int32_t num_categories, int64_t* pq_counts, double* pq_iou, int64_t* flags, void* stream) {
    const osr_status lim = pp_limits("osr_pq_accumulate", num_gt, num_pred);
    if (lim != OSR_OK) return lim;
    OSR_REQUIRE(num_categories >= 1, OSR_ERR_INVALID_ARG, "osr_pq_accumulate: %d categories", num_categories);
    OSR_REQUIRE(counts && pq_counts && pq_iou && flags && (num_gt == 0 || gt_meta) && (num_pred == 0 || pred_slot), OSR_ERR_INVALID_ARG,
                "osr_pq_accumulate: null pointer");
    OSR_REQUIRE(((uintptr_t)counts & 3) == 0 && ((uintptr_t)gt_meta & 3) == 0 && ((uintptr_t)pred_slot & 3) == 0 && ((uintptr_t)pq_counts & 7) == 0 &&
                    ((uintptr_t)pq_iou & 7) == 0 && ((uintptr_t)flags & 7) == 0,
                OSR_ERR_INVALID_ARG, "osr_pq_accumulate: misaligned pointer");
    hipLaunchKernelGGL(pq_accumulate_kernel, dim3(1), dim3(PQ_THREADS), 0, (hipStream_t)stream, counts, num_gt, num_pred, gt_meta, pred_slot, num_categories,
                       pq_counts, pq_iou, flags);
    OSR_CHECK_LAUNCH("osr_pq_accumulate");
    return OSR_OK;
}

// [d2] combine_semantic_and_instance_outputs for one image without host syncs, for gfx950 (include/osr.h: osr_panoptic_combine).
// Six launches whatever the number of instances:
//   1. hipMemsetAsync zeroes the counters of the workspace (areas, row extents, painted bits, histograms).
//   2. pc_pack_kernel, grid-wide: every (k, H, W) mask byte is read once; a wave turns 64 pixels into one 64-bit word with a ballot
//      (pixels in row-major order, words over the linear pixel index), counts the instance's area and finds its first and last row
//      (integer atomics: the sums do not depend on their order).
//   3. pc_walk_kernel, ONE workgroup: ranks the instances by (score descending, index ascending), then walks them in that order over
//      the words of their row range only (a row range is a contiguous word range; every set bit lies inside it, so the result equals
//      the full-plane walk): inter = popcount(mask & painted), the overlap test in double, painted |= mask. Word w is always handled
//      by thread w % 1024, so the painted words need no hand-off between threads. Kept instances go to the segment table.
//   4. pc_paint_kernel, grid-wide: a pixel takes the id of the first kept instance (in walk order) whose bit is set; the others
//      count their label into the unpainted histogram; every pixel counts into the presence histogram (LDS, then integer atomics).
//   5. pc_stuff_kernel, one workgroup: labels 1 .. 255 in ascending order; a label that is present and has at least
//      stuff_area_limit unpainted pixels gets the next id, a table row and an entry of the label -> id table.
//   6. pc_stuff_paint_kernel, grid-wide: the unpainted pixels take their label's id (0 where it has none).
#include "osr_common.h"

#define PC_MAX_K 1024
#define PC_WALK_THREADS 1024
#define PC_LABELS 256

struct PcWorkspace {  // pointers into the caller's workspace
    unsigned long long* packed;   // (k, words)
    unsigned long long* painted;  // (words)
    int* area;                    // (k)
    int* row_lo;                  // (k) max over set pixels of H - y (0: empty)
    int* row_hi;                  // (k) max over set pixels of y + 1
    int* hist;                    // (256) unpainted pixels per label
    int* present;                 // (256) pixels per label
    int* lut;                     // (256) label -> segment id (0: none)
    int* nthings;                 // (1)
};

static int64_t pc_words(int64_t hw) { return (hw + 63) / 64; }

static int64_t pc_layout(int32_t k, int32_t h, int32_t w, char* base, PcWorkspace* ws) {
    const int64_t words = pc_words((int64_t)h * w);
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        char* p = base ? base + off : nullptr;
        off += (bytes + 15) / 16 * 16;
        return p;
    };
    // the zeroed part first: one memset covers [painted, lut)
    char* painted = take(words * 8);
    char* area = take((int64_t)k * 4);
    char* lo = take((int64_t)k * 4);
    char* hi = take((int64_t)k * 4);
    char* hist = take(PC_LABELS * 4);
    char* present = take(PC_LABELS * 4);
    const int64_t zeroed = off;
    char* lut = take(PC_LABELS * 4);
    char* nth = take(16);
    char* packed = take((int64_t)k * words * 8);
    if (ws) {
        ws->painted = (unsigned long long*)painted, ws->area = (int*)area, ws->row_lo = (int*)lo, ws->row_hi = (int*)hi, ws->hist = (int*)hist;
        ws->present = (int*)present, ws->lut = (int*)lut, ws->nthings = (int*)nth, ws->packed = (unsigned long long*)packed;
    }
    (void)zeroed;
    return off;
}

static int64_t pc_zeroed_bytes(int32_t k, int32_t h, int32_t w) {
    const int64_t words = pc_words((int64_t)h * w);
    auto r = [](int64_t b) { return (b + 15) / 16 * 16; };
    return r(words * 8) + 3 * r((int64_t)k * 4) + 2 * r(PC_LABELS * 4);
}

__device__ __forceinline__ int pc_valid_count(const int32_t* count, int k) {
    int kk = count ? *count : k;
    return kk < 0 ? 0 : (kk > k ? k : kk);
}

// grid (ceil(words / 256), k), 256 threads: a wave owns 64 consecutive words
__global__ __launch_bounds__(256) void pc_pack_kernel(const unsigned char* __restrict__ masks, const int32_t* __restrict__ count, int k, int H, int W,
                                                      int64_t words, PcWorkspace ws) {
    const int inst = blockIdx.y;
    if (inst >= pc_valid_count(count, k)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t hw = (int64_t)H * W, w0 = ((int64_t)blockIdx.x * 4 + wave) * 64;
    if (w0 >= words) return;
    const unsigned char* m = masks + (int64_t)inst * hw;
    unsigned long long mine = 0ull;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) {
        const int64_t p = (w0 + j) * 64 + lane;
        const bool b = p < hw && m[p] != 0;
        const unsigned long long bal = __ballot(b);
        if (lane == j) mine = bal;
    }
    const int64_t wi = w0 + lane;
    int area = 0, lo = 0, hi = 0;
    if (wi < words) {
        ws.packed[(int64_t)inst * words + wi] = mine;
        if (mine) {
            area = __popcll(mine);
            const int64_t first = wi * 64 + (__ffsll((long long)mine) - 1), last = wi * 64 + (63 - __clzll((long long)mine));
            lo = H - (int)(first / W);
            hi = (int)(last / W) + 1;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        area += __shfl_xor(area, d, 64);
        lo = max(lo, __shfl_xor(lo, d, 64));
        hi = max(hi, __shfl_xor(hi, d, 64));
    }
    if (lane == 0 && area) {
        atomicAdd(ws.area + inst, area);
        atomicMax(ws.row_lo + inst, lo);
        atomicMax(ws.row_hi + inst, hi);
    }
}

__device__ __forceinline__ int pc_block_sum(int v, int* red) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();  // (red is reused from the previous call)
    if (lane == 0) red[wid] = v;
    __syncthreads();
    int s = 0;
    for (int i = 0; i < PC_WALK_THREADS / 64; ++i) s += red[i];
    return s;
}

// table (cap, 4) int32: isthing, category_id, instance_id (-1 for stuff), area; seg_scores (cap) fp32
__global__ __launch_bounds__(PC_WALK_THREADS) void pc_walk_kernel(const float* __restrict__ scores, const int64_t* __restrict__ classes,
                                                                  const int32_t* __restrict__ count, int k, int H, int W, int64_t words, float overlap_thresh,
                                                                  float conf_thresh, PcWorkspace ws, int32_t* __restrict__ table,
                                                                  float* __restrict__ seg_scores) {
    __shared__ unsigned int key[PC_MAX_K];
    __shared__ int order[PC_MAX_K];
    __shared__ int red[PC_WALK_THREADS / 64];
    const int tid = threadIdx.x;
    const int kk = pc_valid_count(count, k);
    if (tid < kk) key[tid] = osr_float_key(scores[tid]);
    __syncthreads();
    if (tid < kk) {
        const unsigned int mine = key[tid];
        int rank = 0;
        for (int j = 0; j < kk; ++j) rank += (key[j] > mine || (key[j] == mine && j < tid)) ? 1 : 0;
        order[rank] = tid;
    }
    __syncthreads();
    int cur = 0;
    for (int r = 0; r < kk; ++r) {
        const int inst = order[r];
        const float score = scores[inst];
        if (score < conf_thresh) break;  // (uniform: every thread reads the same score)
        const int area = ws.area[inst];
        if (area == 0) continue;
        const int y0 = H - ws.row_lo[inst], y1 = ws.row_hi[inst];  // rows [y0, y1)
        const int64_t wlo = ((int64_t)y0 * W) / 64, whi = ((int64_t)y1 * W + 63) / 64;  // words [wlo, whi)
        const unsigned long long* m = ws.packed + (int64_t)inst * words;
        // thread tid owns the words congruent to tid modulo the workgroup size
        int64_t wfirst = wlo - wlo % PC_WALK_THREADS + tid;
        if (wfirst < wlo) wfirst += PC_WALK_THREADS;
        int inter = 0;
        for (int64_t wi = wfirst; wi < whi; wi += PC_WALK_THREADS) inter += __popcll(m[wi] & ws.painted[wi]);
        inter = pc_block_sum(inter, red);
        if ((double)inter / (double)area > (double)overlap_thresh) continue;
        for (int64_t wi = wfirst; wi < whi; wi += PC_WALK_THREADS) {
            const unsigned long long b = m[wi];
            if (b) ws.painted[wi] |= b;
        }
        if (tid == 0) {
            table[cur * 4 + 0] = 1;
            table[cur * 4 + 1] = (int32_t)classes[inst];
            table[cur * 4 + 2] = inst;
            table[cur * 4 + 3] = area - inter;
            seg_scores[cur] = score;
        }
        ++cur;
    }
    if (tid == 0) *ws.nthings = cur;
}

// grid over pixels, 256 threads
__global__ __launch_bounds__(256) void pc_paint_kernel(const int32_t* __restrict__ labels, int H, int W, int64_t words, PcWorkspace ws,
                                                       const int32_t* __restrict__ table, int32_t* __restrict__ pan) {
    __shared__ int hist[PC_LABELS], present[PC_LABELS];
    for (int i = threadIdx.x; i < PC_LABELS; i += 256) hist[i] = present[i] = 0;
    __syncthreads();
    const int64_t hw = (int64_t)H * W, p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < hw) {
        const int nthings = *ws.nthings;
        const int64_t wi = p >> 6;
        const int bit = (int)(p & 63);
        int id = 0;
        if ((ws.painted[wi] >> bit) & 1ull) {
            for (int s = 0; s < nthings; ++s) {
                const int inst = table[s * 4 + 2];
                if ((ws.packed[(int64_t)inst * words + wi] >> bit) & 1ull) {
                    id = s + 1;
                    break;
                }
            }
        }
        pan[p] = id;
        const int l = labels[p];
        if (l >= 0 && l < PC_LABELS) {
            atomicAdd(present + l, 1);
            if (id == 0) atomicAdd(hist + l, 1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < PC_LABELS; i += 256) {
        if (present[i]) atomicAdd(ws.present + i, present[i]);
        if (hist[i]) atomicAdd(ws.hist + i, hist[i]);
    }
}

__global__ __launch_bounds__(PC_LABELS) void pc_stuff_kernel(PcWorkspace ws, int stuff_area_limit, int32_t* __restrict__ table,
                                                             float* __restrict__ seg_scores, int32_t* __restrict__ seg_count) {
    __shared__ int smem[17];
    const int l = threadIdx.x, nthings = *ws.nthings;
    const int area = ws.hist[l];
    const int kept = (l != 0 && ws.present[l] > 0 && area >= stuff_area_limit) ? 1 : 0;
    int total;
    const int rank = osr_block_excl_scan(kept, smem, &total);
    const int row = nthings + rank;
    ws.lut[l] = kept ? row + 1 : 0;
    if (kept) {
        table[row * 4 + 0] = 0;
        table[row * 4 + 1] = l;
        table[row * 4 + 2] = -1;
        table[row * 4 + 3] = area;
        seg_scores[row] = 0.f;
    }
    if (l == 0) *seg_count = nthings + total;
}

__global__ __launch_bounds__(256) void pc_stuff_paint_kernel(const int32_t* __restrict__ labels, int64_t hw, PcWorkspace ws, int32_t* __restrict__ pan) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    if (pan[p] != 0) return;
    const int l = labels[p];
    if (l > 0 && l < PC_LABELS) {
        const int id = ws.lut[l];
        if (id) pan[p] = id;
    }
}

static bool pc_shape_ok(int32_t k, int32_t h, int32_t w) {
    return k >= 0 && k <= PC_MAX_K && h >= 1 && w >= 1 && (int64_t)h * w <= (1LL << 30);
}

extern "C" int64_t osr_panoptic_combine_workspace_bytes(int32_t k, int32_t h, int32_t w) {
    if (k > PC_MAX_K) {
        osr_set_error("osr_panoptic_combine: at most %d instances per image, got %d", PC_MAX_K, k);
        return OSR_ERR_UNSUPPORTED;
    }
    if (!pc_shape_ok(k, h, w)) {
        osr_set_error("osr_panoptic_combine: k %d, map %d x %d", k, h, w);
        return OSR_ERR_INVALID_ARG;
    }
    return pc_layout(k, h, w, nullptr, nullptr);
}

extern "C" osr_status osr_panoptic_combine(const uint8_t* masks, const float* scores, const int64_t* classes, const int32_t* count, int32_t k,
                                           const int32_t* labels, int32_t h, int32_t w, float overlap_thresh, int32_t stuff_area_limit,
                                           float instances_confidence_thresh, int32_t* panoptic_seg, int32_t* seg_table, float* seg_scores,
                                           int32_t* seg_count, void* workspace, int64_t workspace_bytes, void* stream) {
    const int64_t need = osr_panoptic_combine_workspace_bytes(k, h, w);
    if (need < 0) return (osr_status)need;
    OSR_REQUIRE(labels && panoptic_seg && seg_table && seg_scores && seg_count && workspace, OSR_ERR_INVALID_ARG, "osr_panoptic_combine: null pointer");
    OSR_REQUIRE(k == 0 || (masks && scores && classes), OSR_ERR_INVALID_ARG, "osr_panoptic_combine: null pointer");
    OSR_REQUIRE(workspace_bytes >= need, OSR_ERR_INVALID_ARG, "osr_panoptic_combine: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
    OSR_REQUIRE(((uintptr_t)workspace & 15) == 0, OSR_ERR_UNSUPPORTED, "osr_panoptic_combine: workspace must be 16-byte aligned");
    PcWorkspace ws;
    pc_layout(k, h, w, (char*)workspace, &ws);
    hipStream_t st = (hipStream_t)stream;
    const int64_t hw = (int64_t)h * w, words = pc_words(hw);
    if (hipMemsetAsync(workspace, 0, (size_t)pc_zeroed_bytes(k, h, w), st) != hipSuccess) {
        osr_set_error("osr_panoptic_combine: hipMemsetAsync failed");
        return OSR_ERR_LAUNCH;
    }
    if (k > 0) {
        hipLaunchKernelGGL(pc_pack_kernel, dim3((unsigned)((words + 255) / 256), k), dim3(256), 0, st, masks, count, k, h, w, words, ws);
        OSR_CHECK_LAUNCH("osr_panoptic_combine (pack)");
    }
    hipLaunchKernelGGL(pc_walk_kernel, dim3(1), dim3(PC_WALK_THREADS), 0, st, scores, classes, count, k, h, w, words, overlap_thresh,
                       instances_confidence_thresh, ws, seg_table, seg_scores);
    OSR_CHECK_LAUNCH("osr_panoptic_combine (walk)");
    const unsigned pix_blocks = (unsigned)((hw + 255) / 256);
    hipLaunchKernelGGL(pc_paint_kernel, dim3(pix_blocks), dim3(256), 0, st, labels, h, w, words, ws, seg_table, panoptic_seg);
    OSR_CHECK_LAUNCH("osr_panoptic_combine (paint)");
    hipLaunchKernelGGL(pc_stuff_kernel, dim3(1), dim3(PC_LABELS), 0, st, ws, stuff_area_limit, seg_table, seg_scores, seg_count);
    OSR_CHECK_LAUNCH("osr_panoptic_combine (stuff table)");
    hipLaunchKernelGGL(pc_stuff_paint_kernel, dim3(pix_blocks), dim3(256), 0, st, labels, hw, ws, panoptic_seg);
    OSR_CHECK_LAUNCH("osr_panoptic_combine (stuff paint)");
    return OSR_OK;
}

// How osr_conv2d_fwd covers a layer with the BK=64 kernel (osr_conv_gemm64.hip): the tile configuration and, for a deep-K layer whose
// last dispatch round is mostly empty, the split-K tail. A function of the problem alone -- plain C++, no HIP -- so that the launch,
// osr_conv2d_fwd_describe and osr_conv2d_fwd_workspace_bytes all read ONE plan.
#pragma once
#include "../../include/osr.h"

// Tuning constants. A -DOSR_EXPERIMENT build (never shipped; scripts/ab_*.sh) reads them from the environment instead, so
// that one box can compare settings; the product library has no environment dependence.
#ifdef OSR_EXPERIMENT
#include <stdlib.h>
static int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
#define OSR_KNOB(name, dflt) ([] { static const int v = env_int(name, dflt); return v; }())
#else
#define OSR_KNOB(name, dflt) (dflt)
#endif

// Tile configurations of the plain conv / FC kernel.
enum Conv64Tile { T128x128_1 = 1, T128x128_2, T256x256_2, T128x256_1, T256x128_1, T128x64_1, T128x64_2 };
static int force_tile() { return OSR_KNOB("OSR_CONV_FORCE_TILE", 0); }  // diagnostic: one configuration for every layer it fits

// Tile choice by a small cost model instead of per-layer thresholds. Measured on MI355X (scripts/ab_tiles.sh): with the
// staging pieces interleaved into the MFMA stream every configuration saturates at the same ~4.45 TFLOP/s per CU once a CU
// holds its full complement of workgroups, so what separates them is (i) how many dispatch rounds the grid needs at
// `occ` workgroups per CU (VGPR / LDS limited) and how empty the last round is, and (ii) whether a K slice is bound by
// the matrix pipe (r residents x w) or by the L2 -> LDS latency (single buffer: L + w, double buffer: max(L, r x w)).
//   time = full_rounds x tile(occ) + tile(residents of the last partial round),  tile(r) = fixed + nk x slice(r)
// The 256-wide tiles read the residual in the epilogue (no prefetch under the K loop), which measured 1.6x slower on the
// HBM-bound residual layers: they are not offered to a residual layer with fewer than 18 K slices.
#ifndef C64_BIG_CAP
#define C64_BIG_CAP 5.2e6  // per-CU rate of the 256 x 256 tile under load, FLOP per us
#endif
struct TileCfg { int id, bm, bn, two, occ, pre_res; double cap; };  // cap: per-CU MFMA rate under load, FLOP per us
static const TileCfg kTileCfgs[] = {
    {T128x128_1, 128, 128, 0, 3, 1, 4.45e6}, {T128x128_2, 128, 128, 1, 2, 1, 4.45e6}, {T256x256_2, 256, 256, 1, 1, 0, C64_BIG_CAP},
    {T128x256_1, 128, 256, 0, 2, 0, 4.45e6}, {T256x128_1, 256, 128, 0, 2, 0, 4.45e6}, {T128x64_1, 128, 64, 0, 4, 1, 4.45e6},
    {T128x64_2, 128, 64, 1, 3, 1, 4.45e6},
};
static const TileCfg& conv64_tile(int id) {
    for (const TileCfg& k : kTileCfgs) if (k.id == id) return k;
    return kTileCfgs[0];
}

static double conv64_tile_us(const TileCfg& c, int nk, int residents, bool res) {
    const double kLat = 1.0;  // L2 -> LDS latency of one staged slice (us)
    const double w = (double)c.bm * c.bn * 128.0 / c.cap;  // (the 256 x 256 tile measured 1.61 us per slice on fpn_output2: 5.2 TFLOP/s per CU)
    const double busy = residents * w;
    const double slice = c.two ? (busy > kLat + 0.1 ? busy : kLat + 0.1) : (busy > kLat + w ? busy : kLat + w);
    const double fixed = 1.5 + (c.two ? kLat : 0.0) + (double)c.bm * c.bn / 16384.0 * 1.3 * (res ? 1.5 : 1.0);
    return fixed + nk * slice;
}

// When the caller runs several streams side by side (osr_conv_params.concurrency >= 2: the engine's micro-batch streams) the
// modelled time of the 256 x 256 tile is scaled by 0.8 (OSR_CONV_MODEL_BIG, percent): the empty part of a
// one-workgroup-per-CU round is then filled by the other stream's launches, and the big tile
// moves half the L2 -> LDS and LDS -> register bytes per FLOP of the 128 x 128 tile, which is what counts once both streams
// compete for a CU (same-box end-to-end A/B with the per-configuration rates above: 1.00 -> 1169, 0.85 -> 1221, 0.75 -> 1219,
// 0.65 -> 1208 img/s).
static double model_big_scale() { return OSR_KNOB("OSR_CONV_MODEL_BIG", 80) / 100.0; }

static int conv64_pick_tile(const osr_conv_params& p, long long M, int K) {
    const int nk = K / 64, cout = p.cout;
    const bool res = p.res_mode != 0;
    const int f = force_tile();
    if (f != 0) {
        const bool fits = (f == T256x256_2 || f == T128x256_1) ? cout % 256 == 0 : f == T256x128_1 ? cout % 128 == 0 : true;
        if (fits && !((f == T128x128_2 || f == T128x64_2 || f == T256x256_2) && nk < 2)) return f;
    }
    int best = T128x128_1;
    double best_us = 1e30;
    for (const TileCfg& c : kTileCfgs) {
        if (c.bn == 256 && cout % 256 != 0) continue;
        if (cout <= 64 && c.bn != 64) continue;          // narrow layers: no half-empty N tiles
        // the 256-wide tiles read the residual in the epilogue, unprefetched: not for the short-K (HBM-bound) residual layers. From 18 K slices on
        // (a 3 x 3 layer of >= 128 channels: the data gradients of fpn_output2/3 with their ReLU-mask / gradient-sum epilogues) the epilogue is
        // a few per cent of the tile and the 256 x 256 8-phase loop wins (round 5: fpn_output2's dgrad 1.65 -> 1.2 ms)
        if (res && !c.pre_res && nk < 18) continue;
        if (c.two && nk < 2) continue;
        const long long tiles = (M + c.bm - 1) / c.bm * ((cout + c.bn - 1) / c.bn), slots = 256ll * c.occ;
        const long long full = tiles / slots, rem = tiles % slots;
        double us = (double)full * conv64_tile_us(c, nk, c.occ, res);
        if (rem) us += conv64_tile_us(c, nk, (int)((rem + 255) / 256), res);
        if (c.id == T256x256_2 && p.concurrency >= 2) us *= model_big_scale();
        if (us < best_us) { best_us = us; best = c.id; }
    }
    return best;
}

// rows of a dense (rows, channels) tensor: row m starts at m * channels
static bool conv64_dense_out(const osr_conv_params& p) {
    return p.out_stride_w == p.cout && p.out_stride_h == (long long)p.wo * p.cout && p.out_stride_n == (long long)p.ho * p.wo * p.cout;
}

// ---- split-K of the tail round ---------------------------------------------------------------------------------------
// A grid of T tiles on S = 256 x occ slots runs floor(T / S) full dispatch rounds and one round that is only (T mod S) / S full.
// For a deep-K 1x1 / FC layer (FC1: 1072 tiles of 256 x 256 on 256 slots, 196 K slices: 4.19 rounds, the fifth one 19 % full)
// the partial round is cut along K instead: its tiles go to a second launch in which ksplit workgroups share each tile's K loop
// and write fp32 partial sums, and a small third launch adds them up and applies the epilogue. The partial sums are summed in
// a fixed order: the result does not depend on timing.
struct Conv64Plan {
    TileCfg tile;
    long long tiles_m, tiles_n;
    bool split;  // the fields below hold the split-K tail: the last tail_mtiles rows of M tiles (output rows from m_tail0 on), ksplit workgroups per tile
    int tail_mtiles, ksplit;
    long long m_tail0, ws_bytes;
};

// M, K: rows and depth of the GEMM; stem: the 8-tap stem view; masked: a ReLU mask rides in the epilogue; has_workspace: the caller
// offers a split-K workspace (ws_bytes says how large it must be)
static Conv64Plan conv64_plan(const osr_conv_params& p, long long M, int K, bool stem, bool masked, bool has_workspace) {
    Conv64Plan pl{};
    const TileCfg& c = pl.tile = conv64_tile(conv64_pick_tile(p, M, K));
    const long long tiles_m = pl.tiles_m = (M + c.bm - 1) / c.bm, tiles_n = pl.tiles_n = (p.cout + c.bn - 1) / c.bn;
    if (!has_workspace || stem || p.res_mode != 0 || masked || p.stride_h != 1 || p.stride_w != 1 || p.cin % 64 != 0 || !conv64_dense_out(p)) return pl;
    const int nk = K / 64;
    // the partial sums (tail rows x cout x 4 B x ksplit, written and read once) must be small beside the K loop: 48 slices for a 1 x 1 /
    // FC layer, 32 for a KH x KW convolution (round 4: the 3 x 3 layers of res4 / FPN p4, 1050 tiles of 128 x 128 on 768 slots)
    if (nk < (p.kh * p.kw > 1 ? 32 : 48)) return pl;
    if (c.id != T256x256_2 && c.id != T128x128_1 && c.id != T128x256_1) return pl;  // the tile shapes with a split-K tail instantiation
    const long long tiles = tiles_m * tiles_n, slots = 256ll * c.occ;
    const long long full = tiles / slots, rem = tiles % slots;
    if (full < 1 || rem == 0 || rem * 2 > slots) return pl;
    // a K x K convolution needs at least two full rounds in front of the tail: with one (res4's 3 x 3 layers at batch 16, 1050 tiles on
    // 768 slots) the two extra launches and the partial sums cost more than the half-empty round (measured 100 -> 115 us), with four
    // (fpn_output3 on 256 x 256 tiles) the split takes 380 -> 321 us (scripts/exp_split3x3.py)
    if (p.kh * p.kw > 1 && full < 2) return pl;
    const long long tail_mt = (rem + tiles_n - 1) / tiles_n;  // whole rows of M tiles
    long long ks = slots / (tail_mt * tiles_n);
    if (ks > 8) ks = 8;
    if (ks > nk / 8) ks = nk / 8;
    if (ks < 2) return pl;
    pl.split = true; pl.tail_mtiles = (int)tail_mt; pl.ksplit = (int)ks;
    pl.m_tail0 = (tiles_m - tail_mt) * c.bm;
    pl.ws_bytes = ks * (M - pl.m_tail0) * p.cout * 4;
    return pl;
}

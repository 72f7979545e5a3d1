// Fused MFMA path: the whole Allegro model (forward + hand-derived backward) for a tile of centre
// atoms in ONE kernel launch, float32 compute on the gfx950 matrix cores.
//
// Mapping:
//  * tile  = consecutive centre atoms whose edges fit the edge slots of one workgroup: 4 waves / 64 slots (two
//            independent workgroups per CU, the default) or 8 waves / 128 slots; either way 2 waves per SIMD at
//            <= 256 registers.  Wave w owns slots 16w..16w+15; lane = (slot j = lane & 15, group g = lane >> 4).
//            Persistent workgroups claim chunks of consecutive tiles from a global counter (dynamic schedule).
//  * every per-edge feature vector lives in registers in the v_mfma_f32_16x16x4_f32 C/D layout:
//            tile t, register r of lane (j, g)  <->  feature 16 t + 4 g + r   (4 lanes share one edge).
//            With D = W^T-tile (rows = output features) x activations (cols = edges), register r of an
//            output tile is exactly the B operand of MFMA step r of the next layer: the MLP chains run
//            register-to-register with no LDS traffic and no shuffles.
//  * weights are pre-swizzled on the host into A-operand fragments (one coalesced 1 KiB dwordx4 load
//            feeds 4 MFMAs) and laid out as ONE stream in the exact order a tile consumes them (forward
//            weights, then the transposed copies in backward order), so the prefetch ring is a running pointer.
//  * the two-body embedding x0(d; type pair) is read from a per-pair cubic spline table built from the float64
//            MLP and its exact derivative (fused_prepare); option fused_tb=mlp evaluates it in the kernel.
//  * the only cross-edge coupling -- the per-centre environment sum and its gradient -- goes through
//            an LDS staging tile [slots][128 features] and a deterministic per-atom reduction.
//  * activations needed by the backward pass are stored as raw register images in a per-wave
//            private scratch (written and re-read by the same wave within the same tile: Infinity-Cache traffic).
//  * arithmetic of the linears (option fused_arith): f32-input MFMA; f16x2 (two float16 terms per operand, three f16-MFMA
//            products, f32 accumulate: fused_h.h); bf16x3 (exact 3-way bf16 split, six bf16-MFMA terms); tf32eq (two bf16 terms,
//            only for model files that set allow_tf32).
//
// Supported model shape (fused_shapes.h decides; others run the wide kernels or the generic path): l_max = 1, up to 32 tensor features (33..64: k_fused_lx2 on the lifted
// model), up to 64 scalars, MLP width up to 64 (65..128: the WT = 8 instances, zero-padded to 128), read-out width up to 32 (33..64: the RT = 4 instances, zero-padded to 64; narrower than the kernel's fixed 32 / 64 / 64 or 128 / 32 or 64: zero-padded by the host, model_io.cpp: pad_host_model),
// MLPs of 2 hidden layers x 64 (1 or 3 hidden layers on the f16x2 instances with the tabulated two-body embedding: template parameter MD, round 5),
// read-out 1 x 32 (2 x 32 on the same f16x2 instances: template parameter RD), <= 3 layers, <= 16 types; any number of Bessel functions and any cutoff-polynomial order (the radial basis only
// enters through the tabulated two-body embedding; fused_tb=mlp needs 8).  Reference graph:
// the TorchScript model executed at /root/reference/pair_nequip_allegro.cpp:409-430.
#include <hip/hip_runtime.h>

#include <cmath>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "../../include/allegro_hip.h"
#include "engine.h"
// weight fragments in flight per wave: 4 (two steps ahead) instead of the wide kernels' 8 -- the 16 registers are worth more to this kernel than the deeper prefetch
// (1 M-atom Si: 58.3 -> 56.8 ms; 2 fragments: slower than 4)
#define AHIP_RING 4
#include "fused_common.h"
#include "fused_h.h"
#include "fused_rows.h"
#include "prims.h"

// This file is compiled in parts (Makefile; same options, divides the build time): AHIP_FUSED_PART 0 = the host side + the instances of part 0, n = the instances of
// part n alone; which instances a part holds is fused_shapes.h: FUSED_INSTANCES.  (Rounds 2-3 gave part 1 other compiler options because it computed wrong
// forces with part 0's: that was the store-data hazard described at fused_common.h: bstore, not the options.)
#ifndef AHIP_FUSED_PART
#define AHIP_FUSED_PART 0
#endif
namespace ahip {


// Two workgroup shapes (template parameter NW = waves per workgroup, 16 edge slots per wave):
//   NW = 4: 64-slot tiles, <= 6 centres, ~79 KB LDS -> TWO independent workgroups per CU.  Their barriers are
//           independent, so the two waves of a SIMD drift into different phases and one wave's MFMA chains run
//           under the other's tensor-product / reduction / memory phases.  Default.
//   NW = 8: 128-slot tiles, <= 12 centres, ~159 KB LDS, one workgroup per CU: for lists with 65..128 edges per centre.
[[maybe_unused]] static constexpr int MAX_TILE_SLOTS = 128;
static constexpr int MAXNL = 3;
static constexpr int STG_LD = 132;       // staging leading dimension: all 128 features of a slot; 16-byte aligned rows
static constexpr int ENV_LD = 132;       // per-atom environment row (the tensor product reads it as float4)


struct FusedArgs {
  // edge list
  const int *eoff, *e_ii, *e_j;
  const unsigned char *e_tt;     // per edge: (model type of centre) << 4 | (model type of neighbour)
  const int2 *centre;            // per centre ii: {atom index ilist[ii], model type}
  const float *rvec;
  const double *rcut;            // [T*T]
  int T, NL, p;
  float cenv;
  // tiles
  unsigned int *tile_counter;
  int tchunk;                    // tiles per claim of the dynamic schedule (1 for small systems: a workgroup's last claim sets the makespan)    // dynamic tile schedule (zeroed by k_pack_finish)
  const int *tile_a0, *tile_e0, *ntiles;   // tile t = centres [tile_a0[t], tile_a0[t+1]), edges [tile_e0[t], tile_e0[t+1])
  const int *maxdeg_sel;         // null, or the device word with the list's largest degree: the 4-wave shape runs iff it is <= 64, the 8-wave shape iff not (fused_run)
  // weights (offsets in floats into wbase)
  const float *wbase;
  int wbytes;
  int o_stream;                  // the per-tile weight-fragment stream (consumption order)
  int o_tbtab, tb_nk;            // tabulated two-body embedding: [pair][tb_nk intervals][tile 4][coef 4][16] cubic coefficients
  int o_tpl, o_pair, o_out1, o_scale, o_shift;
  int o_res[MAXNL];
  // scratch
  float *scratch;
  long long wg_scratch, wave_scratch;     // floats
  // outputs
  double *f, *eatom, *partial;            // partial [gridDim.x][7]
  long long *prof;                        // [PH_N] or unused
  float *dbg;                             // [E][8] per-edge diagnostics or null
  float cp[6];                            // cutoff polynomial: a, b, c of f = 1 - a x^p + b x^(p+1) - c x^(p+2) and a p, b (p + 1), c (p + 2) of its derivative (scalar registers, not per-lane values held over a tile)
  int *err;                               // host-mapped word: set when an edge gradient comes out non-finite (float16 range exceeded)
  double *vatom;                          // [nall][9] per-atom virial (the VA instances only)
  int env_bwd;                            // option env_backward (Model::EnvBackward): 0 auto, 1 centre, 2 edge -- the environment backward linear once per centre or per edge
};

template <int NW, int NL = MAXNL, int RT = 2> struct __attribute__((aligned(16))) Lds {
  static constexpr int SLOTS = 16 * NW;
  static constexpr int MAXA = NW == 4 ? 6 : 12;   // centre atoms per tile (LDS budget)
  float stage[SLOTS * STG_LD];
  float env[NL][MAXA * ENV_LD];
  float denv[MAXA * ENV_LD];
  float tp[NL][5 * 32];                   // tensor-product path weights [layer][path][u]
  float park[NW][8 * ROW];                // per-wave private park: V^{k+1} forward, dE/dV backward ([lm][t] images)
  double eacc[MAXA];                      // energy accumulated over this workgroup's tiles, per centre slot (one owner thread each)
  double virw[NW][6];                     // virial accumulated per wave (owner: lanes 0..5 of the wave)
  int aoff[2][MAXA + 2];                  // slot offsets of the tile's centres, double-buffered by tile parity
  float rc[16];                           // model cutoff table [T*T] for T <= 4 (more types: read from A.rcut, the LDS budget of two workgroups per CU is spent)
  float scale[16], shift[16];             // per-type energy scale / shift
  float res[NL][2];                       // residual update coefficients per layer
  int chunk[2];                           // first tile of the current / next claimed chunk
  float wo1[RT == 2 ? 32 : 4]; __device__ __forceinline__ float *wo1v() { if constexpr (RT == 2) return wo1; else return tp[NL - 1] + 64; }      // the read-out's final 32 -> 1 vector: read in every tile (a global load there drained the vector-memory queue behind `za`).  RT = 4: the 64 -> 1 vector lives in tp[NL - 1][64 .. 127] instead, the last layer's path weights of the paths with l = 1 output, which no tile reads (the last layer computes its scalar outputs only); another 128 B here would put the 4-wave, 3-layer instance at 81 936 B, 16 B over half a CU's LDS: one workgroup per CU instead of two
};

// ---------------------------------------------------------------------------- device helpers

// scratch row map (per wave, rows of 1 KiB): fused_rows.h
// per layer: omega 4 | silu' of the MD hidden layers of the latent MLP, WT each | u 4 | V_in 8   (MD = latent MLP depth, 1..3; WT = 16-feature tiles of a hidden layer, 4 or 8; MD = 2, WT = 4: the reference YAML's, 24 rows)

static constexpr float C_S3 = 1.7320508075688772f;
static constexpr float C_P1 = 0.5773502691896258f;     // (1,1,0): sqrt(1) * w3j = 1/sqrt(3)
static constexpr float C_P4 = 0.7071067811865476f;     // (1,1,1): sqrt(3) * w3j = eps_ijk / sqrt(2)

// ---- bf16x3 arithmetic: every f32 value is split EXACTLY into three bf16 terms (truncation: 8+8+8 significant
// bits), x = hi + mid + lo, and a product w*x is evaluated on the bf16 matrix cores as the six terms of weight
// 2^-16 and above:  w_hi x_hi + w_hi x_mid + w_mid x_hi + w_hi x_lo + w_mid x_mid + w_lo x_hi  (each bf16 product is
// exact in f32, accumulation is f32; the dropped terms are <= 3 * 2^-24 |w x|, the size of one f32 rounding).  One
// v_mfma_f32_16x16x32_bf16 (16 cycles on the matrix core, which -- unlike the f32-input MFMA -- runs beside the
// VALU) contracts 32 input features, so a K-step is a PAIR of 16-feature tiles: lane (j, g) supplies its 4
// registers of tile 2s and of tile 2s+1 as the 8 k-slots of its lane group.  The C/D layout is the same as the
// f32 form, so the register chaining of the f32 kernel carries over unchanged.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
struct Bop { u32x4 hi, mid, lo; };           // B operand of one K-step: 8 bf16 per lane and term

__device__ __forceinline__ f32x4 mfma_b(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// two f32 -> packed bf16 terms (low half = first value)
__device__ __forceinline__ void split2(float v0, float v1, unsigned &hi, unsigned &mid, unsigned &lo) {
  const unsigned a = __builtin_bit_cast(unsigned, v0), b = __builtin_bit_cast(unsigned, v1);
  hi = __builtin_amdgcn_perm(b, a, 0x07060302u);
  const float r0 = v0 - __builtin_bit_cast(float, a & 0xffff0000u), r1 = v1 - __builtin_bit_cast(float, b & 0xffff0000u);
  const unsigned ra = __builtin_bit_cast(unsigned, r0), rb = __builtin_bit_cast(unsigned, r1);
  mid = __builtin_amdgcn_perm(rb, ra, 0x07060302u);
  const float q0 = r0 - __builtin_bit_cast(float, ra & 0xffff0000u), q1 = r1 - __builtin_bit_cast(float, rb & 0xffff0000u);
  lo = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, q1), __builtin_bit_cast(unsigned, q0), 0x07060302u);
}
__device__ __forceinline__ Bop split_pair(const f32x4 &t0, const f32x4 &t1) {
  Bop b;
  unsigned h, m, l;
  split2(t0[0], t0[1], h, m, l); b.hi[0] = h; b.mid[0] = m; b.lo[0] = l;
  split2(t0[2], t0[3], h, m, l); b.hi[1] = h; b.mid[1] = m; b.lo[1] = l;
  split2(t1[0], t1[1], h, m, l); b.hi[2] = h; b.mid[2] = m; b.lo[2] = l;
  split2(t1[2], t1[3], h, m, l); b.hi[3] = h; b.mid[3] = m; b.lo[3] = l;
  return b;
}

// Streamed linear on the bf16x3 arithmetic.  in: KS K-steps (pairs of 16-feature tiles, already split); out: NT f32
// tiles through the same epilogue functors as linear_s; SPLIT additionally emits the outputs as the next linear's
// B operands (outb[p] = tiles 2p, 2p+1).  Fragments per (tile pair p, K-step): hi0 hi1 mid0 mid1 lo0 lo1, 1 KiB each,
// in consumption order; RINGB of them are in flight (a multiple of 6: every linear consumes a multiple of 6).
static constexpr int RINGB = 12;              // fragments in flight, three-term split (2 steps of 6)
static constexpr int RINGB2 = 8;              // two-term split (2 steps of 4): every linear of the tile sequence consumes a multiple of 8 fragments except the four mixing blocks (4 each, alternating phase) -- a deeper ring would need the per-layer fragment count to be a multiple of it
template <int NTERM> struct RingB { static constexpr int N = NTERM == 3 ? RINGB : RINGB2; };
// NTERM = 3: the float32-equivalent split above (six products).  NTERM = 2 ("tf32eq", used only when the model file sets allow_tf32,
// the reference's own licence for TF32-class arithmetic, pair_nequip_allegro.cpp:267-270): hi + mid of both operands, the three products
// w_hi x_hi + w_hi x_mid + w_mid x_hi; the dropped terms are <= 3 * 2^-17 |w x| (TF32 itself rounds both operands to 2^-11), the weight
// stream is 4 fragments per step = the bytes of the f32 stream, and all of it runs on the bf16 matrix cores beside the VALU.
template <int KS, int NT, bool ACC, bool SPLIT, int RP, class Epi, int NTERM = 3>
__device__ __forceinline__ void linear_b(__amdgpu_buffer_rsrc_t W, int &wp, const Bop (&in)[KS], f32x4 (&out)[NT], Bop (&outb)[NT / 2],
                                         int v16, u32x4 (&ring)[RingB<NTERM>::N], Epi epi) {
  static_assert(NT % 2 == 0, "output tiles are processed in pairs");
  static_assert(NTERM == 2 || NTERM == 3, "two or three bf16 terms per operand");
  constexpr int RB = RingB<NTERM>::N;
  constexpr int NF = 2 * NTERM;                       // fragments per step: term-major, two output tiles each
  constexpr int NPROD = NTERM == 3 ? 6 : 3, MF = 2 * NPROD;      // products per accumulator, MFMAs per step
  constexpr int NP = NT / 2, NSTEP = NP * KS, NS = NF * NSTEP;
  f32x4 acc0, acc1, prev0, prev1;
  // byte offset of the next fragments to request: ONE running scalar advanced step by step, as in linear_s (written as wp + constant the optimiser
  // forms every offset of the tile at the top of the tile loop and spills them to VGPR lanes: 508 scalar spills in the two-layer instance)
  int wo = (wp + RB * 256) * 4;
  pin_s(wo);
#pragma unroll
  for (int s = 0; s < NSTEP; ++s) {
    const int p = s / KS, ks = s % KS;
    if (ks == 0) {
      if (ACC) { acc0 = out[2 * p]; acc1 = out[2 * p + 1]; }
      else { acc0 = f32x4{0.f, 0.f, 0.f, 0.f}; acc1 = f32x4{0.f, 0.f, 0.f, 0.f}; }
    }
    u32x4 a[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      a[i] = ring[(RP + NF * s + i) % RB];
      ring[(RP + NF * s + i) % RB] = __builtin_bit_cast(u32x4, bload_w(W, v16 + (i & 3) * 1024, wo + (i >> 2) * 4096));      // + k KiB: the instruction's immediate offset
    }
    wo += NF * 1024;
    pin_s(wo);
    // the two accumulators alternate; smallest terms first
#pragma unroll
    for (int m = 0; m < NPROD; ++m) {
      // NTERM 3, term m: (weight term, activation term) = (lo,hi) (mid,mid) (hi,lo) (mid,hi) (hi,mid) (hi,hi);  NTERM 2: (mid,hi) (hi,mid) (hi,hi)
      const int wt = NTERM == 3 ? (m == 0 ? 2 : (m == 1 || m == 3) ? 1 : 0) : (m == 0 ? 1 : 0);
      const int xt = NTERM == 3 ? ((m == 0 || m == 3 || m == 5) ? 0 : (m == 1 || m == 4) ? 1 : 2) : (m == 1 ? 1 : 0);
      const u32x4 bx = xt == 0 ? in[ks].hi : xt == 1 ? in[ks].mid : in[ks].lo;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        if (hh == 0) acc0 = mfma_b(a[2 * wt], bx, acc0);
        else acc1 = mfma_b(a[2 * wt + 1], bx, acc1);
        if (p > 0) {
          // the 8 epilogue elements of the previous pair are spread over the KS * MF MFMAs of this pair
          const int idx = ks * MF + 2 * m + hh, tot = KS * MF;
          const int e0 = (idx * 8 + tot - 1) / tot, e1 = ((idx + 1) * 8 + tot - 1) / tot;
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (e >= e0 && e < e1) {
              if (e < 4) out[2 * (p - 1)][e] = epi.apply(2 * (p - 1), e, prev0[e]);
              else out[2 * (p - 1) + 1][e - 4] = epi.apply(2 * (p - 1) + 1, e - 4, prev1[e - 4]);
              if (e == 7) {
                epi.flush(2 * (p - 1));
                if (SPLIT) outb[p - 1] = split_pair(out[2 * (p - 1)], out[2 * (p - 1) + 1]);
              }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (ks == KS - 1) {
      epi.tile_done(2 * p, acc0);
      epi.tile_done(2 * p + 1, acc1);
      if (p == NP - 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { out[2 * p][r] = epi.apply(2 * p, r, acc0[r]); out[2 * p + 1][r] = epi.apply(2 * p + 1, r, acc1[r]); }
        epi.flush(2 * p);
        if (SPLIT) outb[p] = split_pair(out[2 * p], out[2 * p + 1]);
      } else { prev0 = acc0; prev1 = acc1; }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  wp += NS * 256;
  pin_s(wp);
}
template <int RB> __device__ __forceinline__ void ring_prime_b(__amdgpu_buffer_rsrc_t W, int wp, int v16, u32x4 (&ring)[RB]) {
  int wo = wp * 4;
  pin_s(wo);
#pragma unroll
  for (int j = 0; j < RB; ++j) ring[j] = __builtin_bit_cast(u32x4, bload_w(W, v16 + (j & 3) * 1024, wo + (j >> 2) * 4096));
}

// Per-centre sum of the staged tile: dst[a][f] = scale * sum_{slots of a} stage[slot][f], f < 128.
// 128 features x (NW/2) atoms per pass; 4 independent accumulators keep 4 LDS reads in flight.
template <int NW, int NL, int RT> __device__ __forceinline__ void reduce_stage(const Lds<NW, NL, RT> &lds, const int *aoff, float *dst, int na, float scale, int tid) {
  const int fidx = tid & 127;
  for (int a = tid >> 7; a < na; a += NW / 2) {
    const int s0 = aoff[a], s1 = aoff[a + 1];
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
    int sl = s0;
    for (; sl + 4 <= s1; sl += 4) {
      acc0 += lds.stage[sl * STG_LD + fidx];
      acc1 += lds.stage[(sl + 1) * STG_LD + fidx];
      acc2 += lds.stage[(sl + 2) * STG_LD + fidx];
      acc3 += lds.stage[(sl + 3) * STG_LD + fidx];
    }
    for (; sl < s1; ++sl) acc0 += lds.stage[sl * STG_LD + fidx];
    dst[a * ENV_LD + fidx] = scale * ((acc0 + acc1) + (acc2 + acc3));
  }
}
// ---------------------------------------------------------------------------- the kernel
// PROF: opt-in phase timing (s_memtime stamps per wave, summed into A.prof[phase]); AHIP_FUSED_PROF=1.
enum { PH_GEOM = 0, PH_TB, PH_EMB, PH_ENV, PH_TP, PH_MIX, PH_LAT, PH_OUT, PH_BLAT, PH_BMIX, PH_BTP, PH_BENV, PH_BEMB, PH_BTB, PH_FIN, PH_N };
#define PHASE(id) do { if (PROF) { long long _t = clock64(); pacc[id] += _t - tprev; tprev = _t; } } while (0)

// One weight-fragment ring per arithmetic (see linear_s / linear_b); lin<> dispatches a linear of the tile sequence to
// the f32-input MFMA form or to the bf16x3 form (inputs are split into their three bf16 terms right here).
// AR: arithmetic of the tile's linears: 0 = f32-input MFMA, 1 = bf16x3 (three-term split, float32-equivalent), 2 = tf32eq (two-term bf16 split),
// 3 = f16x2 (two float16 terms, float32-equivalent inside float16's exponent range: fused_h.h)
// MX: the f16x2 operand split in its mixed-precision-fma form (fused_h.h: split2_h), chosen per instance by k_fused.
template <int AR, bool MX = false> struct RingT {
  int act = 1;                 // wave-uniform: 0 while the wave's 16 slots of the current tile hold no edge (its linears are skipped, see the tile loop)
  f32x4 f[AR != 0 ? 1 : RING];
  u32x4 b[AR == 0 ? 1 : (AR == 1 ? RINGB : AR == 2 ? RINGB2 : RINGH)];
};
// BR = false: the caller has tested ring.act itself, around a PAIR of one-step linears (see lin_mix).
// jump: f16x2 only, see linear_h (the stream jump over a linear this wave will skip).
template <int AR, int KT, int NT, bool ACC, int RPI, bool BR = true, class Epi, bool MX>
__device__ __forceinline__ void lin(__amdgpu_buffer_rsrc_t W, int &wp, const f32x4 (&in)[KT], f32x4 (&out)[NT], int v16, RingT<AR, MX> &ring, Epi epi, int jump = 0) {
  if (BR && !ring.act) {             // (uniform) a wave without edges in this tile: no fragments, no MFMAs, no epilogue; finite outputs for the arithmetic around the linears
    if constexpr (!ACC) {
#pragma unroll
      for (int t = 0; t < NT; ++t) out[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    return;
  }
  if constexpr (AR == 3) {
    static_assert(KT % 2 == 0, "K-steps are pairs of 16-feature tiles");
    Hop b[1][KT / 2], unused[1][NT / 2];
#pragma unroll
    for (int ks = 0; ks < KT / 2; ++ks) b[0][ks] = split_pair_h<MX>(in[2 * ks], in[2 * ks + 1]);
    Epi ep[1] = {epi};
    linear_h<1, KT / 2, NT, ACC, false, (4 * RPI) % RINGH, Epi, true>(W, wp, b, reinterpret_cast<f32x4 (&)[1][NT]>(out), unused, v16, ring.b, ep, jump);
  } else if constexpr (AR != 0) {
    static_assert(KT % 2 == 0, "K-steps are pairs of 16-feature tiles");
    constexpr int NTERM = AR == 1 ? 3 : 2;
    Bop b[KT / 2], unused[NT / 2];
#pragma unroll
    for (int ks = 0; ks < KT / 2; ++ks) b[ks] = split_pair(in[2 * ks], in[2 * ks + 1]);
    // ring phase: RPI counts the four 32x32 channel-mixing blocks, which consume less than a ring each (2 * NTERM fragments)
    linear_b<KT / 2, NT, ACC, false, (2 * NTERM * RPI) % RingB<NTERM>::N, Epi, NTERM>(W, wp, b, out, unused, v16, ring.b, epi);
  } else {
    linear_s<KT, NT, ACC, (4 * RPI) % RING, Epi>(W, wp, in, out, v16, ring.f, epi);
  }
}

// The three m components of an l = 1 row share ONE channel-mixing matrix: on the f16x2 arithmetic they go through the linear as three GROUPS that share every weight
// fragment (linear_h<3, ...>: one fragment load, three B operands, three accumulator sets) instead of three passes over three copies of the matrix in the stream:
// 8 KiB of fragments fewer per mixing block and direction and wave-tile.
template <int RPI, bool BR = true, class Epi, bool MX>
__device__ __forceinline__ void lin_m3(__amdgpu_buffer_rsrc_t W, int &wp, const f32x4 (&in0)[2], const f32x4 (&in1)[2], const f32x4 (&in2)[2], f32x4 (&out)[3][2], int v16,
                                       RingT<3, MX> &ring, Epi (&epi)[3], int jump = 0) {
  if (BR && !ring.act) {
#pragma unroll
    for (int q = 0; q < 3; ++q) { out[q][0] = f32x4{0.f, 0.f, 0.f, 0.f}; out[q][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    return;
  }
  Hop b[3][1], unused[3][1];
  b[0][0] = split_pair_h<MX>(in0[0], in0[1]); b[1][0] = split_pair_h<MX>(in1[0], in1[1]); b[2][0] = split_pair_h<MX>(in2[0], in2[1]);
  linear_h<3, 1, 2, false, false, (4 * RPI) % RINGH, Epi, true>(W, wp, b, out, unused, v16, ring.b, epi, jump);
}
// A channel mixing on the f16x2 arithmetic is two ONE-step linears (the l = 0 block, then lin_m3).  They share one `ring.act` branch: a region that consumes a whole
// ring (two steps) leaves every slot at the age it had on entry, whichever way the branch went.  With a branch each, the path "first skipped, second taken" -- which
// never runs, a wave is idle for a whole tile, but which the wait-count insertion has to merge -- presents the second linear's fragments as the youngest loads of the
// queue, and its first products wait behind s_waitcnt vmcnt(3..2) for everything older.
template <class Epi0, class Epi3, bool MX>
__device__ __forceinline__ void lin_mix(__amdgpu_buffer_rsrc_t W, int &wp, const f32x4 (&in0)[2], const f32x4 (&in1)[2], const f32x4 (&in2)[2], const f32x4 (&in3)[2], f32x4 (&out0)[2],
                                        f32x4 (&out)[3][2], int v16, RingT<3, MX> &ring, Epi0 epi0, Epi3 (&epi)[3], int jump = 0) {
  if (!ring.act) {
    out0[0] = f32x4{0.f, 0.f, 0.f, 0.f}; out0[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 3; ++q) { out[q][0] = f32x4{0.f, 0.f, 0.f, 0.f}; out[q][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    return;
  }
  lin<3, 2, 2, false, 0, false>(W, wp, in0, out0, v16, ring, epi0, jump);       // (both one-step linears request fragments of the linear behind the pair)
  lin_m3<1, false>(W, wp, in1, in2, in3, out, v16, ring, epi, jump);
}

// MD: hidden layers of the latent MLP (allegro_mlp_hidden_layers_depth of /root/reference/tests/test_data/test_repro_allegro.yaml:94; 2 there).  1 and 3 exist for the
// f16x2 instances with the tabulated two-body embedding (round 5: the fused family widened by one axis); every MD-dependent piece below is `if constexpr`.
// What a tile reads from the edge lists: bounds (scalar), this lane's edge slot, this thread's centre, one slot offset.
struct TileIn {
  int a0, a1, e0, e1;
  float rx, ry, rz;
  int eii, jat, tt;
  int eoff;
};
// The fetch is a REQUEST: nothing in it waits on the vector-memory queue, which holds the weight ring and the saved rows of the linear it runs under.
//  - tile_bounds: the four bounds through SCALAR loads (the addresses are wave-uniform and the packing kernels wrote the arrays before this launch: the constant
//    address space is what lets the compiler pick s_load_dword in a kernel that also stores).  Called a tile's length ahead of tile_fetch, their wait is lgkmcnt.
//  - tile_fetch: per-edge and per-centre entries through range-checked buffer loads whose descriptors start at the tile's first edge / centre and end at its last:
//    no branch (the join of an exec-masked branch gets s_waitcnt vmcnt(0)), a lane beyond the tile -- or any lane of a tile >= ntiles, whose bounds are 0 -- reads
//    nothing and receives 0.  The one default that is not 0 (rx = 1: a finite unit vector for idle slots) is applied where the values are consumed.
struct TileBounds { int a0, a1, e0, e1; };
typedef const __attribute__((address_space(4))) int *cint_p;
__device__ __forceinline__ TileBounds tile_bounds(const FusedArgs &A, int tile, int ntiles) {
  const int tc = max(min(tile, ntiles - 1), 0);       // (uniform) a readable entry for every tile; both arrays hold at least two words
  const cint_p ta = (cint_p)(unsigned long long)A.tile_a0, te = (cint_p)(unsigned long long)A.tile_e0;
  TileBounds b = {ta[tc], ta[tc + 1], te[tc], te[tc + 1]};
  if (tile >= ntiles) b = TileBounds{0, 0, 0, 0};
  return b;
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t list_rsrc(const void *base, long long first_byte, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void *)((unsigned long long)base + (unsigned long long)first_byte), 0, bytes, 0x00020000);
}
__device__ __forceinline__ void tile_fetch(const FusedArgs &A, const TileBounds &b, int s, int tid, TileIn &n) {
  n.a0 = b.a0; n.a1 = b.a1; n.e0 = b.e0; n.e1 = b.e1;
  const int ne = b.e1 - b.e0, na = b.a1 - b.a0;       // (uniform) <= tile slots, <= MAXA
  const int eb = b.e0 & 3;                            // the byte list's descriptor starts on a dword
  const __amdgpu_buffer_rsrc_t RV = list_rsrc(A.rvec, 12ll * b.e0, 12 * ne), EI = list_rsrc(A.e_ii, 4ll * b.e0, 4 * ne), EJ = list_rsrc(A.e_j, 4ll * b.e0, 4 * ne),
                               ET = list_rsrc(A.e_tt, b.e0 - eb, ne + eb), EO = list_rsrc(A.eoff, 4ll * b.a0, na > 0 ? 4 * (na + 1) : 0);
  n.rx = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(RV, 12 * s, 0, 0));           // (three dwords: the 96-bit form of the builtin compiles to ONE dword here)
  n.ry = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(RV, 12 * s + 4, 0, 0));
  n.rz = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(RV, 12 * s + 8, 0, 0));
  n.eii = (int)__builtin_amdgcn_raw_buffer_load_b32(EI, 4 * s, 0, 0);
  n.jat = (int)__builtin_amdgcn_raw_buffer_load_b32(EJ, 4 * s, 0, 0);
  n.tt = (int)__builtin_amdgcn_raw_buffer_load_b8(ET, s + eb, 0, 0);
  n.eoff = (int)__builtin_amdgcn_raw_buffer_load_b32(EO, 4 * tid, 0, 0);
}

// VA: also the per-atom virial (output "atomic_virial"); instances launched only while that output is registered, so the default ones keep their code.  RD: hidden layers of the read-out MLP (1; 2 on f16x2 + table only, built in fused_hr.o)
// WT: 16-feature tiles of one hidden layer of the latent MLP: 4 (MLP width <= 64), or 8 (65..128, zero-padded to 128: f16x2 + table, read-out depth 1, not profiled; built in fused_hm.o).
// Only the hidden vectors z, z2 / dh, du and their saved rows grow: no LDS array, table, latent x or environment row depends on it, so the LDS (two workgroups per CU at NW = 4) is the same.  RT: 16-feature tiles of the read-out MLP's hidden layer: 2 (read-out width <= 32), or 4 (33..64, zero-padded to 64: f16x2 + table, WT = 4, read-out depth 1, not profiled; built in fused_hq.o): only the read-out vectors (zr, dzr) and the final R -> 1 vector in LDS (Lds::wo1v: inside the path-weight table, no byte more) grow, the two folded linears of the last layer become 64 x 64 blocks like every other linear of a WT = 4 instance, and the row maps and the per-wave scratch do not depend on it (the f16x2 instances save no z (W3 Wr) rows).
template <int NW, bool PROF, int AR, bool TBT, int NLT, int MD = 2, bool VA = false, int RD = 1, int WT = 4, int RT = 2>
__global__ void __launch_bounds__(NW * 64, 2) k_fused(FusedArgs A) {
  constexpr int NTHREADS = NW * 64, MAXA = Lds<NW>::MAXA;
  // f16x2 instances (round 5): the last hidden layer of the latent MLP saves its RAW pre-activation rows and the layer's output rows u are not saved at all: the backward
  // pass needs u only for <u, g> (the cutoff gradient), and <u, g> = <silu(z), g W^T> falls out of its first linear's epilogue (EpiMulSiluZ), which rebuilds silu and silu'
  // from z -- 6 row stores and 6 row loads fewer per wave-tile of a two-layer model for ~10 VALU operations per value there: 45.8 -> 44.4 ms at 1 M Si atoms.
  constexpr bool SAVEZ = AR == 3;
  constexpr bool PARKV = true;             // (round 6; its A/B: profiles/r06_a_ab_k_fused_rows_and_spills.txt, 39.7 -> 37.8 ms)
  // The LAST layer's activation rows (silu' / pre-activations of its last two hidden layers) live in the wave's own slots of the staging tile instead of scratch rows:
  // the tile is idle from that layer's environment sum to its backward tensor product (EpiSiluSaveDL / EpiSiluSaveZL): 8 row stores and 8 row loads fewer per wave-tile.
  constexpr bool STGROWS = true;           // (36.0 -> 34.3 ms)
  // WT = 8: a slot's staging row (128 floats = 8 images) holds ONE 128-wide hidden layer, so only the last hidden layer is parked there (images 0..7); the one below it
  // goes to the wave's scratch rows like a non-last layer's
  constexpr bool STG2 = WT == 4;           // the hidden layer below the last is parked as well (images 0..3; the last one then sits in images ZQ = 4..7)
  constexpr int ZQ = WT == 4 ? 4 : 0;
  constexpr int OZL = R_OZ(MD, WT), OU = R_OU(MD, WT), OVIN = R_OVIN(MD, WT);      // row offsets inside a layer: silu' of the LAST hidden layer, u, V_in (MD = 2, WT = 4: 8, 12, 16)
  static_assert(WT == 4 || (WT == 8 && AR == 3 && TBT && !PROF && RD == 1), "MLP width 128: f16x2 instances with the two-body table only, read-out depth 1, not profiled");
  // every linear whose shape depends on WT consumes whole rings of the weight stream, so the ring phases (RPI) of everything behind it are those of WT = 4
  static_assert(lin_frags_h(6, WT) % RINGH == 0 && lin_frags_h(WT, WT) % RINGH == 0 && lin_frags_h(WT, 4) % RINGH == 0 && lin_frags_h(4, WT) % RINGH == 0 && lin_frags_h(WT, 6) % RINGH == 0 &&
                    lin_frags_h(WT, 2) % RINGH == 0 && lin_frags_h(2, WT) % RINGH == 0,
                "the weight ring stays in phase");
  static_assert(RT == 2 || (RT == 4 && AR == 3 && TBT && !PROF && RD == 1 && WT == 4), "read-out width 64: f16x2 instances with the two-body table only, MLP width 64, read-out depth 1, not profiled");
  static_assert(lin_frags_h(WT, RT) % RINGH == 0 && lin_frags_h(4, RT) % RINGH == 0 && lin_frags_h(RT, 4) % RINGH == 0 && lin_frags_h(RT, WT) % RINGH == 0, "the weight ring stays in phase");
  static_assert(MD >= 1 && MD <= 3 && (MD == 2 || (AR == 3 && TBT)), "latent MLP depth 1 / 3: f16x2 instances with the two-body table only");
  static_assert(RD == 1 || (RD == 2 && AR == 3 && TBT && !PROF), "read-out depth 2: f16x2 instances with the two-body table only, not profiled");
  __shared__ Lds<NW, NLT, RT> lds;
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 15, g = lane >> 4, wave = tid >> 6;
  const int v16 = lane * 16;
  // wave-uniform buffer descriptors (made provably uniform with readfirstlane)
  __amdgpu_buffer_rsrc_t SB, WB;
  {
    unsigned long long b = (unsigned long long)(A.scratch + (size_t)blockIdx.x * A.wg_scratch + (size_t)wave * A.wave_scratch);
    unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    SB = __builtin_amdgcn_make_buffer_rsrc((void *)(((unsigned long long)hi << 32) | lo), 0, (int)(A.wave_scratch * 4), 0x00020000);
    WB = __builtin_amdgcn_make_buffer_rsrc((void *)A.wbase, 0, A.wbytes, 0x00020000);
  }
  if (A.maxdeg_sel && ((*A.maxdeg_sel <= 64) != (NW == 4))) return;     // both shapes were launched: the tiles were packed for the other one
  const float *__restrict__ Wb = A.wbase;
  for (int k = tid; k < A.NL * 160; k += NTHREADS) {      // path weights with their CG constants folded in
    const int pth = (k % 160) / 32;
    if (RT != 2 && k >= (NLT - 1) * 160 + 64) continue;   // (RT = 4: the unread tail of the last layer's rows holds the read-out's final vector, Lds::wo1v)
    lds.tp[k / 160][k % 160] = Wb[A.o_tpl + k] * (pth == 1 ? C_P1 : pth == 4 ? C_P4 : 1.f);
  }
  const int ntiles = *A.ntiles;
  // The layer count is a template parameter and both layer loops are unrolled: "last layer" is then a compile-time fact (the folded
  // read-out below has a different shape there), nothing is carried around a loop edge, and the register allocation of each layer
  // is its own.  With a run-time loop the same fold cost more in spills than its 64 MFMAs saved (64.3 -> 67.7 ms; unrolled: 61.0).
  constexpr int NL = NLT;
  double acc_part = 0.0;       // thread 0: energy; threads 64..69: virial components
  long long pacc[PH_N];
  long long tprev = 0;
  const long long t_clk0 = clock64(), t_wall0 = wall_clock64();
  if (PROF) {
#pragma unroll
    for (int k = 0; k < PH_N; ++k) pacc[k] = 0;
    tprev = clock64();
  }
  float *const pk0 = lds.park[wave];
  // (the mixed-fma operand split, fused_h.h, where it leaves every instance's registers and scratch as they were: the 4-wave tiles of MLP width <= 64)
  RingT<AR, AR == 3 && NW == 4 && WT == 4> ring;      // the weight-fragment stream (see linear_s / linear_b)
  int wp = A.o_stream;
  if constexpr (AR != 0) ring_prime_b(WB, wp, v16, ring.b);
  else ring_prime(WB, wp, v16, ring.f);
  if (tid < MAXA) lds.eacc[tid] = 0.0;
  if (lane < 6) lds.virw[wave][lane] = 0.0;
  if (A.T <= 4 && tid < A.T * A.T) lds.rc[tid] = (float)A.rcut[tid];
  if (tid < A.T) { lds.scale[tid] = Wb[A.o_scale + tid]; lds.shift[tid] = Wb[A.o_shift + tid]; }
  if (tid < 2 * A.NL) lds.res[tid >> 1][tid & 1] = Wb[A.o_res[tid >> 1] + (tid & 1)];
  if constexpr (RT == 2) { if (tid >= 64 && tid < 96) lds.wo1[tid - 64] = Wb[A.o_out1 + tid - 64]; }
  else { if (tid >= 64 && tid < 64 + 16 * RT) lds.wo1v()[tid - 64] = Wb[A.o_out1 + tid - 64]; }

  const int s = wave * 16 + j;                 // this lane's edge slot
  float *const st = lds.stage + s * STG_LD;
  // Dynamic tile schedule: workgroups claim chunks of TCHUNK consecutive tiles from a global counter (workgroup
  // speeds differ by +-12 % across the chip, a static round-robin leaves the slowest one 13 % behind the average).
  // The next chunk is claimed while the first tile of the current one runs.
  if (tid == 0) lds.chunk[0] = (int)atomicAdd(A.tile_counter, (unsigned)A.tchunk);
  __syncthreads();
  int par = 0, cpar = 0, ck = 0;
  int cbase = __builtin_amdgcn_readfirstlane(lds.chunk[0]);

  TileIn nx_;
  tile_fetch(A, tile_bounds(A, cbase, ntiles), s, tid, nx_);
  asm volatile("" : "+v"(nx_.rx), "+v"(nx_.ry), "+v"(nx_.rz), "+v"(nx_.eii), "+v"(nx_.jat), "+v"(nx_.tt), "+v"(nx_.eoff));       // landed before the loop is entered, as on its back edge (the finish waits for them in front of the force atomics): one queue state at the tile top

  for (;;) {
    const int tile = cbase + ck;
    if (tile >= ntiles) break;
    int claimed = 0;
    if (ck == 0 && tid == 0) {
      // The counter's address goes through a vector register the optimiser cannot see through: with a provably uniform address the atomic is rewritten into a
      // wave-wide reduction whose result is broadcast by v_readfirstlane right behind it, i.e. behind s_waitcnt vmcnt(0).  One lane runs this; the returned value is
      // first touched at the `lds.chunk` write below, a whole phase later.
      // (A GLOBAL atomic: a flat one makes every later wait a vmcnt(0).)
      unsigned long long tcnt = (unsigned long long)A.tile_counter;
      asm volatile("" : "+v"(tcnt));
      claimed = (int)__hip_atomic_fetch_add((__attribute__((address_space(1))) unsigned int *)tcnt, (unsigned)A.tchunk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // Everything a tile reads from the lists is ONE level of loads behind the (scalar) tile bounds: the edge
    // build packs the type pair per edge and k_tile_info the centre index/type, so no dependent chain
    // (edge -> centre -> type) is exposed here.  The whole set was requested a phase before the previous tile ended (tile_fetch below).
    const int a0 = nx_.a0, a1 = nx_.a1, e0 = nx_.e0, e1 = nx_.e1;
    // A wave whose 16 slots lie behind the tile's last edge (one 33..48-edge centre in a 64-slot tile: Li3PO4, 45 % of the tiles) skips every linear of the tile
    // (lin: ring.act) and addresses its saved rows out of range (loads return 0, stores are dropped); it still takes part in the barriers and in the per-centre
    // reductions, which never read its slots.  Its stream position needs no repair: a tile ends with wp = stream start and the ring holding the stream's first
    // fragments, which is what the wave's ring has held since its last active tile.
    // The branch pays twice.  Li3PO4 (102 400 atoms): 9.30 -> 7.77 ms.  And 1 M Si, where no wave is ever empty (56 of 64 slots): 44.7 -> 39.7 ms -- the same with
    // a condition that is always true (profiles/r05_w_last_experiments.md §6): a wave-uniform branch around each linear makes it a scheduling / allocation region of
    // its own (spills of the headline instance 304 -> 120 B per lane).  The wide kernels lose with the same branch (fused_lx2: 20.3 -> 21.9 ms): their linears are
    // ordered by hand across each other.
    // (the per-centre instances, CEN below, form the wave index per tile, as a scalar, from an opaque copy of the thread index: what hangs on it -- the slot range, the
    // park rows, the table offset, the virial partials -- is then not held across the tile loop; with the per-centre form in the kernel those four values went to scratch)
    constexpr bool CEN = AR == 3 && NW == 4;
    int tq = tid, lq_ = lane, wvq = wave;
    if constexpr (CEN) {
      asm volatile("" : "+v"(tq));
      wvq = __builtin_amdgcn_readfirstlane(tq >> 6);
      lq_ = tq & 63;
    }
    float *const pk = CEN ? lds.park[wvq] : pk0;
    const int wact = __builtin_amdgcn_readfirstlane(e0 + wvq * 16 < e1 ? 1 : 0);
    ring.act = wact;
    const int v16t = wact ? v16 : 0x7ffffff0;
    const int na = a1 - a0;
    // Environment backward once per CENTRE (f16x2, 4 waves).  The transposed environment linear acts on dom_e = [d0_i ; Y1_e d1_i + Y2_e d2_i + Y3_e d3_i], and
    // d0..d3 (lds.denv) belong to the centre: dom_e W^T = P0_i + Y1_e P1_i + Y2_e P2_i + Y3_e P3_i with four 64-vectors P per centre.  A tile of <= 3 centres has
    // <= 12 of them, one wave's 16 MFMA columns: wave 0 (which always holds edges) runs the linear on them, the other waves skip it -- 16 KiB of fragments and 48 MFMAs
    // fewer per wave and layer -- and every lane combines its centre's four vectors from LDS.  Tiles of 4..6 centres take the per-edge linear.
    // cen (wave-uniform): 0 per edge; 1 this wave computes P; 2 this wave skips the linear; 3 a wave without edges (barrier only).
    int cen = 0;
    if constexpr (CEN) {
      if (A.env_bwd != 2 && na <= 3) cen = !wact ? 3 : wvq == 0 ? 1 : 2;
    }
    // The skipping waves JUMP the stream (form (a) of the two ways to keep their ring in phase): the last RINGH requests of the linear in front of the skipped one -- the
    // backward channel mixing, or the last layer's dcat linear -- read 16 fragments further on, so the ring holds the first fragments of the linear behind it.
    const int cjump = cen == 2 ? 16 * 1024 : 0;
    par ^= 1;
    int *const aoffp = lds.aoff[par];
    const int e = e0 + s;
    const bool valid = e < e1;
    const float rx = valid ? nx_.rx : 1.f, ry = nx_.ry, rz = nx_.rz;      // (a slot beyond the tile's edges fetched zeros: tile_fetch)
    const int aloc = valid ? nx_.eii - a0 : 0, jat = nx_.jat, ti = nx_.tt >> 4, tj = nx_.tt & 15;
    if (tid <= na) aoffp[tid] = nx_.eoff - e0;
    // ---------------- geometry ----------------
    const float d = sqrtf(rx * rx + ry * ry + rz * rz);
    const float inv = 1.f / d;
    const float nx = rx * inv, ny = ry * inv, nz = rz * inv;
    const float rc = A.T <= 4 ? lds.rc[ti * A.T + tj] : (float)A.rcut[ti * A.T + tj];
    const float xx = d / rc;
    float fc, dfc_dx;
    cutoff_poly_c(A.p, A.cp, xx, fc, dfc_dx);
    if (!valid) { fc = 0.f; dfc_dx = 0.f; }
    const float Y1 = C_S3 * ny, Y2 = C_S3 * nz, Y3 = C_S3 * nx;
    const float pref = 2.f / rc;
    const float PI = 3.14159265358979323846f;
    const float *const envrow = lds.env[0] + aloc * ENV_LD;        // + kk * MAXA*ENV_LD
    const float *const denvrow = lds.denv + aloc * ENV_LD;
    PHASE(PH_GEOM);

    // ---------------- two-body embedding x0(d; type pair) ----------------
    f32x4 x[4];
    float tb_t = 0.f, tb_invh = 0.f;
    if constexpr (TBT) {
      // x0 depends on the edge only through (d, t_i, t_j): the MLP [one-hots, Bessel * cutoff] -> 64 -> 64 -> 64, times the
      // cutoff, is tabulated per type pair as piecewise cubics in d (Hermite data from the float64 MLP and its exact
      // derivative, host side: fused_prepare).  Interpolation error (h^4 |4th derivative| / 384 at 512 intervals) is below
      // float32 rounding; it replaces 3 + 3 linears (18 % of the MFMAs), their SiLU epilogues and 12 saved rows per wave-tile.
      tb_invh = (float)A.tb_nk / rc;
      const float sft = d * tb_invh;
      const int kq = min((int)sft, A.tb_nk - 1);
      tb_t = sft - (float)kq;
      // the entry's byte offset inside the weight buffer (32 bits per lane; the 16 gathers differ in the instruction's immediate offset)
#ifdef ABL_NOTBGATHER   // timing experiment only (results are wrong): every edge reads the same table entry
      const int tb_off = (A.o_tbtab + 4 * g) * 4;
#else
      const int tb_off = (A.o_tbtab + ((ti * A.T + tj) * A.tb_nk + kq) * 256 + 4 * (lq_ >> 4)) * 4;       // (lq_ >> 4 = g)
#endif
      const float vm = (valid && xx < 1.f) ? 1.f : 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f32x4 c0 = bload_w(WB, tb_off + (t * 4 + 0) * 64, 0), c1 = bload_w(WB, tb_off + (t * 4 + 1) * 64, 0);
        const f32x4 c2 = bload_w(WB, tb_off + (t * 4 + 2) * 64, 0), c3 = bload_w(WB, tb_off + (t * 4 + 3) * 64, 0);
        x[t] = (c0 + tb_t * (c1 + tb_t * (c2 + tb_t * c3))) * vm;
        // d x0 / dd for the backward pass: one coalesced row now instead of three per-edge gathers then
        // (gathering the entry again in the backward pass instead of saving these four rows -- 12 gathers for 4 stores + 4 loads -- was measured in round 6: 33.5 vs 33.2 ms)
        bstore(SB, v16t, (R_Z1TB() + t) * ROW * 4, (c1 + tb_t * (2.f * c2 + (3.f * tb_t) * c3)) * (vm * tb_invh));
      }
    } else {
      f32x4 z[4], z2[4];
      {
        const float *pt = Wb + A.o_pair + (size_t)(ti * A.T + tj) * 64;
#pragma unroll
        for (int t = 0; t < 4; ++t) z[t] = *(const f32x4 *)(pt + 16 * t + 4 * g);
      }
      f32x4 bfin[2];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float n = (float)(4 * g + r + 1);
        // Bessel numbers 9..16 (groups 2,3) meet zero weight rows; revolutions: sin(pi n x)
        bfin[0][r] = g < 2 ? pref * __builtin_amdgcn_sinf(0.5f * n * xx) * inv * fc : 0.f;
        bfin[1][r] = 0.f;
      }
      lin<AR, 2, 4, true, 0>(WB, wp, bfin, z, v16t, ring, EpiSiluSaveD{SB, R_Z1TB(), v16t});
      lin<AR, 4, 4, false, 0>(WB, wp, z, z2, v16t, ring, EpiSiluSaveD{SB, R_Z2TB(), v16t});
      lin<AR, 4, 4, false, 0>(WB, wp, z2, x, v16t, ring, EpiSaveScale{{SB, R_U0(), v16t}, fc});
    }
    PHASE(PH_TB);
    // ---------------- tensor embedding weights (V^0 = w0 (x) Y is rebuilt where needed) -------------
    {
      f32x4 w0[4];
      // w0 goes to scratch (backward) and to the LDS park rows 0..3, where layer 0 picks it up
      lin<AR, 4, 4, false, 0>(WB, wp, x, w0, v16t, ring, EpiSavePark{{SB, R_W0(), v16t}, pk, 0, lane});
    }
    if (ck == 0 && tid == 0) lds.chunk[cpar ^ 1] = claimed;
    __syncthreads();          // aoff visible; previous tile's LDS users done
    // the NEXT tile's bounds, requested a whole tile before tile_fetch builds its descriptors from them (the next chunk's first tile has just been published)
    const TileBounds nb_ = tile_bounds(A, (ck + 1 == A.tchunk) ? __builtin_amdgcn_readfirstlane(lds.chunk[cpar ^ 1]) : tile + 1, ntiles);
    PHASE(PH_EMB);

    // ---------------- layers, forward ----------------
    f32x4 zr[RT];              // read-out pre-activations: produced by the last layer (see its latent MLP)
#pragma unroll
    for (int kk = 0; kk < NL; ++kk) {
      const bool last = (kk == NL - 1);
      const int RL = R_LAYER(kk, MD, WT);
      float *const envk = lds.env[0] + kk * (MAXA * ENV_LD);
      f32x4 V[4][2];
      {
        f32x4 om[4];
        lin<AR, 4, 4, false, 0>(WB, wp, x, om, v16t, ring, EpiSaveFrom2{{SB, RL + 0, v16t}});      // rows RL + 2, RL + 3: the l = 1 weights, all the backward pass reads
        // environment sum over the centre's edges
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          float *sp = st + 16 * t + 4 * g;                   // features 16 t + 4 g + (0..3): one 16-byte store per component
          *(f32x4 *)(sp) = om[t];
          *(f32x4 *)(sp + 32) = om[2 + t] * Y1;
          *(f32x4 *)(sp + 64) = om[2 + t] * Y2;
          *(f32x4 *)(sp + 96) = om[2 + t] * Y3;
        }
        __syncthreads();
        reduce_stage(lds, aoffp, envk, na, A.cenv, tid);
        __syncthreads();
      }
      if (kk == 0) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const f32x4 w1 = park_load(pk, 2 + t, lane);
          V[0][t] = park_load(pk, t, lane);
          V[1][t] = w1 * Y1; V[2][t] = w1 * Y2; V[3][t] = w1 * Y3;
        }
      } else {
#pragma unroll
        for (int lm = 0; lm < 4; ++lm)
#pragma unroll
          for (int t = 0; t < 2; ++t) V[lm][t] = park_load(pk, 2 * lm + t, lane);   // V^{kk} parked by the previous layer's mix
      }
      __builtin_amdgcn_sched_barrier(0);
      PHASE(PH_ENV);
      // tensor product
      f32x4 Vp[4][2];
      {
        const float *en = envrow + kk * (MAXA * ENV_LD);
        const float *tp = lds.tp[kk];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          // float4 arithmetic over the lane's 4 features of this tile: register pairs go to v_pk_* as they are
          const int b = 16 * t + 4 * g;
          const f32x4 e0v = *(const f32x4 *)(en + b), e1v = *(const f32x4 *)(en + 32 + b), e2v = *(const f32x4 *)(en + 64 + b),
                      e3v = *(const f32x4 *)(en + 96 + b);
          const f32x4 v0 = V[0][t], v1 = V[1][t], v2 = V[2][t], v3 = V[3][t];
          Vp[0][t] = *(const f32x4 *)(tp + b) * v0 * e0v + *(const f32x4 *)(tp + 32 + b) * (v1 * e1v + v2 * e2v + v3 * e3v);
          if (!last) {
            const f32x4 p2 = *(const f32x4 *)(tp + 64 + b), p3 = *(const f32x4 *)(tp + 96 + b), c4 = *(const f32x4 *)(tp + 128 + b);
            const f32x4 p2v0 = p2 * v0, p3e0 = p3 * e0v;
            Vp[1][t] = p2v0 * e1v + p3e0 * v1 + c4 * (v2 * e3v - v3 * e2v);
            Vp[2][t] = p2v0 * e2v + p3e0 * v2 + c4 * (v3 * e1v - v1 * e3v);
            Vp[3][t] = p2v0 * e3v + p3e0 * v3 + c4 * (v1 * e2v - v2 * e1v);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      PHASE(PH_TP);
      // channel mixing -> V^{kk+1}: saved in the next layer's VIN rows and parked in LDS
      if (!last) {
        f32x4 o2[2];
        if constexpr (AR == 3) {
          // f16x2: the l = 0 block, then the l = 1 block once for its three components (lin_m3)
          f32x4 o3[3][2];
          if (PARKV && kk + 1 == NL - 1) {                 // (the LAST layer's input tensor is not saved: see below)
            EpiPark ep[3] = {EpiPark{pk, 2, lane}, EpiPark{pk, 4, lane}, EpiPark{pk, 6, lane}};
            lin_mix(WB, wp, Vp[0], Vp[1], Vp[2], Vp[3], o2, o3, v16t, ring, EpiPark{pk, 0, lane}, ep);
          } else {
            EpiSavePark ep[3] = {EpiSavePark{{SB, R_LAYER(kk + 1, MD, WT) + OVIN + 2, v16t}, pk, 2, lane}, EpiSavePark{{SB, R_LAYER(kk + 1, MD, WT) + OVIN + 4, v16t}, pk, 4, lane},
                                 EpiSavePark{{SB, R_LAYER(kk + 1, MD, WT) + OVIN + 6, v16t}, pk, 6, lane}};
            lin_mix(WB, wp, Vp[0], Vp[1], Vp[2], Vp[3], o2, o3, v16t, ring, EpiSavePark{{SB, R_LAYER(kk + 1, MD, WT) + OVIN + 0, v16t}, pk, 0, lane}, ep);
          }
        } else if (PARKV && kk + 1 == NL - 1) {
          // the LAST layer's input tensor is not saved: nothing writes the park between its forward tensor product and its backward one (the last layer has
          // no channel mixing), so the backward pass reads it from there -- 8 row stores and 8 row loads fewer per wave-tile
          lin<AR, 2, 2, false, 0>(WB, wp, Vp[0], o2, v16t, ring, EpiPark{pk, 0, lane});
          lin<AR, 2, 2, false, 1>(WB, wp, Vp[1], o2, v16t, ring, EpiPark{pk, 2, lane});
          lin<AR, 2, 2, false, 2>(WB, wp, Vp[2], o2, v16t, ring, EpiPark{pk, 4, lane});
          lin<AR, 2, 2, false, 3>(WB, wp, Vp[3], o2, v16t, ring, EpiPark{pk, 6, lane});
        } else {
          lin<AR, 2, 2, false, 0>(WB, wp, Vp[0], o2, v16t, ring, EpiSavePark{{SB, R_LAYER(kk + 1, MD, WT) + OVIN + 0, v16t}, pk, 0, lane});
          lin<AR, 2, 2, false, 1>(WB, wp, Vp[1], o2, v16t, ring, EpiSavePark{{SB, R_LAYER(kk + 1, MD, WT) + OVIN + 2, v16t}, pk, 2, lane});
          lin<AR, 2, 2, false, 2>(WB, wp, Vp[2], o2, v16t, ring, EpiSavePark{{SB, R_LAYER(kk + 1, MD, WT) + OVIN + 4, v16t}, pk, 4, lane});
          lin<AR, 2, 2, false, 3>(WB, wp, Vp[3], o2, v16t, ring, EpiSavePark{{SB, R_LAYER(kk + 1, MD, WT) + OVIN + 6, v16t}, pk, 6, lane});
        }
      }
      PHASE(PH_MIX);
      // latent MLP
      {
        f32x4 cat[6], z[WT], z2[WT];
        cat[0] = x[0]; cat[1] = x[1]; cat[2] = x[2]; cat[3] = x[3]; cat[4] = Vp[0][0]; cat[5] = Vp[0][1];
        // hidden layer h (1..MD) saves silu'(z), the last one its raw z on the f16x2 instances (SAVEZ); in the last layer of the model the rows of hidden layers
        // MD - 1 and MD go to the staging tile (images 0..3 and 4..7) instead of scratch (WT = 8: those of hidden layer MD alone, images 0..7: STG2, ZQ)
        const bool stg = STGROWS && last;
        float *const sq = st + 4 * g;
#define AHIP_HIDDEN(KT, IN, OUT, H) do { \
          if (stg && (H) >= (STG2 ? MD - 1 : MD)) { \
            if (SAVEZ && (H) == MD) lin<AR, KT, WT, false, 0>(WB, wp, IN, OUT, v16t, ring, EpiSiluSaveZL{sq, ZQ}); \
            else lin<AR, KT, WT, false, 0>(WB, wp, IN, OUT, v16t, ring, EpiSiluSaveDL{sq, (H) == MD ? ZQ : 0}); \
          } else if (SAVEZ && (H) == MD) lin<AR, KT, WT, false, 0>(WB, wp, IN, OUT, v16t, ring, EpiSiluSaveZ{SB, RL + R_OZ(H, WT), v16t}); \
          else lin<AR, KT, WT, false, 0>(WB, wp, IN, OUT, v16t, ring, EpiSiluSaveD{SB, RL + R_OZ(H, WT), v16t}); } while (0)
        AHIP_HIDDEN(6, cat, z, 1);
        if constexpr (MD >= 2) AHIP_HIDDEN(WT, z, z2, 2);
        if constexpr (MD >= 3) AHIP_HIDDEN(WT, z2, z, 3);
#undef AHIP_HIDDEN
        f32x4 (&zl)[WT] = MD == 2 ? z2 : z;             // output of the last hidden layer
        const float ra = lds.res[kk][0], rbf = lds.res[kk][1] * fc;
        if (!last) {
          f32x4 xn[4];
          if constexpr (SAVEZ) lin<AR, WT, 4, false, 0>(WB, wp, zl, xn, v16t, ring, EpiResidualNS<4>{x, ra, rbf});
          else lin<AR, WT, 4, false, 0>(WB, wp, zl, xn, v16t, ring, EpiResidual<4>{{SB, RL + OU, v16t}, x, ra, rbf});
          x[0] = xn[0]; x[1] = xn[1]; x[2] = xn[2]; x[3] = xn[3];
        } else {
          // Last layer: its new latent x' = ra x + rb fc (z2 W3) feeds nothing but the read-out's first linear, and no non-linearity
          // sits between the two, so  x' Wr = ra (x Wr) + rb fc (z2 (W3 Wr))  with W3 Wr multiplied out by the host in float64: two
          // 64 -> 32 linears instead of a 64 -> 64 and a 64 -> 32 one, here and (transposed) in the backward pass: 64 of the tile's
          // 1472 MFMAs per wave and two saved rows less.  z2 first: it dies there.  (RT = 4: two 64 -> 64 linears instead of three)
          if constexpr (RT == 2) {
            f32x4 za[2], up[2];
            if constexpr (SAVEZ) lin<AR, WT, 2, false, 0>(WB, wp, zl, up, v16t, ring, EpiNone{});
            else lin<AR, WT, 2, false, 0>(WB, wp, zl, up, v16t, ring, EpiSave{SB, RL + OU, v16t});
            lin<AR, 4, 2, false, 0>(WB, wp, x, za, v16t, ring, EpiNone{});
            zr[0] = ra * za[0] + rbf * up[0]; zr[1] = ra * za[1] + rbf * up[1];
          } else {
            // 64 wide, the two terms meet in the accumulators: zr = rbf (z2 (W3 Wr)) out of the first linear's epilogue, then += (ra x) Wr -- no za / up beside zr (32
            // registers this kernel does not have); x is dead behind this linear (the backward pass has its own dx), so it is scaled in place
            static_assert(SAVEZ, "read-out width 64: f16x2 instances (no z2 (W3 Wr) rows saved)");
            lin<AR, WT, RT, false, 0>(WB, wp, zl, zr, v16t, ring, EpiScale{rbf});
#pragma unroll
            for (int t = 0; t < 4; ++t) x[t] = ra * x[t];
            lin<AR, 4, RT, true, 0>(WB, wp, x, zr, v16t, ring, EpiNone{});
          }
        }
      }
      PHASE(PH_LAT);
    }

    // ---------------- read-out ----------------
    // saved rows are requested one linear ahead of their first use all through the backward pass (their
    // round trip is an L2 miss: ~2 us): u and z2 of the last layer now, under the read-out MFMAs
    f32x4 upre[4], zt[WT], w0h[2];
#pragma unroll
    for (int t = 0; t < RT; ++t) if (!SAVEZ) upre[t] = bload(SB, v16t, (R_LAYER(NL - 1, MD, WT) + OU + t) * ROW * 4);      // the last layer saved RT rows: z2 (W3 Wr)
    if (!STGROWS) load_rows<WT>(SB, R_LAYER(NL - 1, MD, WT) + OZL, zt, v16t);
    __builtin_amdgcn_sched_barrier(0);
    f32x4 zr2[RT];             // RD = 2: pre-activations of the read-out's second hidden layer
    if constexpr (RD == 2) {
      f32x4 hr[RT];
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) hr[t][r] = silu1(zr[t][r]);
      lin<AR, RT, RT, false, 0>(WB, wp, hr, zr2, v16t, ring, EpiNone{});
    }
    f32x4 (&zo)[RT] = RD == 2 ? zr2 : zr;       // pre-activations of the last hidden layer
    f32x4 wo1[RT];             // the read-out's final R -> 1 vector (out.w1, or out.w2 of a depth-2 read-out)
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      if constexpr (RT == 2) wo1[t] = *(const f32x4 *)(lds.wo1 + 16 * t + 4 * g);
      else wo1[t] = *(const f32x4 *)(lds.wo1v() + 16 * t + 4 * g);
    }
    float eps = 0.f;
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) eps += silu1(zo[t][r]) * wo1[t][r];
    eps = gsum(eps);
    asm volatile("" : "+v"(eps));            // computed here, not sunk to its use at the end of the tile (keeps the read-out rows alive until then)

    // =========================== backward ===========================
    // f16x2: the backward pass is linear in this upstream gradient and runs scaled by a power of two that brings it to O(1) (float16 has no exponent range to spare)
    // ... PER CENTRE TYPE (round 6): the exponent of this centre type's own upstream gradient, so that species whose energy scales differ by orders of
    // magnitude each run at O(1); every edge of a centre shares it, which is all the per-centre sums need.  Its inverse waits in the slot's pad floats of
    // the staging tile (st[128]: never staged, never reduced) instead of a register held to the end of the tile.
    float bsc = 1.f;
    if constexpr (AR == 3) {
      int bex;
      (void)frexpf(lds.scale[ti] * A.cenv, &bex);
      bex = min(max(bex, -100), 100);         // a subnormal or huge scale (bex ~ -130 for 1e-39) would make one of 2^-bex, 2^bex inf: both stay finite and normal
      bsc = ldexpf(1.f, -bex);
      if (g == 0) st[128] = ldexpf(1.f, bex);
    }
    const float deps = valid ? lds.scale[ti] * A.cenv * bsc : 0.f;
    f32x4 dx[4];
    f32x4 dzr[RT];
    if constexpr (RT != 2) {
      // the 64-wide vector is not held across the read-out (k_fused sits at 256 registers): read again, through a pointer the optimiser cannot see through
      const float *wq = lds.wo1v() + 4 * (lq_ >> 4);       // (lq_ >> 4 = g)
      asm volatile("" : "+v"(wq));
#pragma unroll
      for (int t = 0; t < RT; ++t) wo1[t] = *(const f32x4 *)(wq + 16 * t);
    }
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) dzr[t][r] = deps * wo1[t][r] * dsilu1(zo[t][r]);
    if constexpr (RD == 2) {
      // dzr holds the gradient of zr2: back through out.w1^T (the second half-ring block) and the first hidden layer's SiLU; linear in deps, so the f16x2 scale passes through
      f32x4 dhr[RT];
      lin<AR, RT, RT, false, 1>(WB, wp, dzr, dhr, v16t, ring, EpiNone{});
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) dzr[t][r] = dhr[t][r] * dsilu1(zr[t][r]);
    }
    lin<AR, RT, 4, false, 0>(WB, wp, dzr, dx, v16t, ring, EpiNone{});              // dzr Wr^T = the gradient w.r.t. x' of the last layer
    if (STGROWS) {                                                                 // the last layer's rows of its last hidden layer, from the staging tile
#pragma unroll
      for (int t = 0; t < WT; ++t) zt[t] = stg_load(st + 4 * g, ZQ + t);
    }
    float dfc_part = 0.f, dY1 = 0.f, dY2 = 0.f, dY3 = 0.f;
    PHASE(PH_OUT);

#pragma unroll
    for (int kk = NL - 1; kk >= 0; --kk) {
      const bool last = (kk == NL - 1);
      const int RL = R_LAYER(kk, MD, WT);
      f32x4 dVp[4][2], Vk[4][2], W0b[4];
      {
        f32x4 du[WT], dh[WT];
        f32x4 zt1[WT];
        if (!last && SAVEZ) {
          // the u rows are not saved: <u, g> = <silu(z), g W^T> comes out of the first backward linear's epilogue (EpiMulSiluZ), whose input is the unscaled gradient
          const float ra = lds.res[kk][0], rb = lds.res[kk][1];
          if constexpr (MD >= 2) load_rows<WT>(SB, RL + OZL - WT, zt1, v16t);
          __builtin_amdgcn_sched_barrier(0);
          float ug = 0.f;
          lin<AR, 4, WT, false, 0>(WB, wp, dx, dh, v16t, ring, EpiMulSiluZ<WT>{zt, rb * fc, ug});
          dfc_part += rb * ug;
#pragma unroll
          for (int t = 0; t < 4; ++t) dx[t] = ra * dx[t];
        } else if (last && SAVEZ) {
          const float ra = lds.res[kk][0], rb = lds.res[kk][1];
          if constexpr (MD >= 2) { if (!(STGROWS && STG2)) load_rows<WT>(SB, RL + OZL - WT, zt1, v16t); }      // (WT = 8: the staging row holds the last hidden layer alone)
          __builtin_amdgcn_sched_barrier(0);
          float ug = 0.f;
          lin<AR, RT, WT, false, 0>(WB, wp, dzr, dh, v16t, ring, EpiMulSiluZ<WT>{zt, rb * fc, ug});
          dfc_part += rb * ug;
#pragma unroll
          for (int t = 0; t < 4; ++t) dx[t] = ra * dx[t];
        } else if (!last) {
          if constexpr (!SAVEZ) {             // (the instances that save u rows: WT = 4)
          const float ra = lds.res[kk][0], rb = lds.res[kk][1];
          f32x4 accv = upre[0] * dx[0];
#pragma unroll
          for (int t = 1; t < 4; ++t) accv += upre[t] * dx[t];
          const float rbfc = rb * fc;
#pragma unroll
          for (int t = 0; t < 4; ++t) { du[t] = rbfc * dx[t]; dx[t] = ra * dx[t]; }
          dfc_part += rb * ((accv[0] + accv[1]) + (accv[2] + accv[3]));
          if constexpr (MD >= 2) load_rows<4>(SB, RL + OZL - 4, zt1, v16t);                  // silu' of the hidden layer below the last: first used 96 MFMAs from here
          __builtin_amdgcn_sched_barrier(0);
          lin<AR, 4, 4, false, 0>(WB, wp, du, dh, v16t, ring, EpiMulRows<4>{zt});
          }
        } else {
          if constexpr (!SAVEZ) {
          // last layer (read-out folded in, see the forward pass): upre = the two rows z2 (W3 Wr); the z2 gradient comes straight
          // from dzr through (W3 Wr)^T
          static_assert(SAVEZ || RT == 2, "the instances that save the z2 (W3 Wr) rows have read-out width 32");
          const float ra = lds.res[kk][0], rb = lds.res[kk][1];
          const f32x4 accv = upre[0] * dzr[0] + upre[1] * dzr[1];
          const float rbfc = rb * fc;
          f32x4 du2[2];
#pragma unroll
          for (int t = 0; t < 2; ++t) du2[t] = rbfc * dzr[t];
#pragma unroll
          for (int t = 0; t < 4; ++t) dx[t] = ra * dx[t];
          dfc_part += rb * ((accv[0] + accv[1]) + (accv[2] + accv[3]));
          if constexpr (MD >= 2) { if (!STGROWS) load_rows<4>(SB, RL + OZL - 4, zt1, v16t); }
          __builtin_amdgcn_sched_barrier(0);
          lin<AR, 2, 4, false, 0>(WB, wp, du2, dh, v16t, ring, EpiMulRows<4>{zt});
          }
        }
        if constexpr (MD >= 2) {
          if (STGROWS && STG2 && last) {                         // silu' of the hidden layer below the last, from the staging tile
#pragma unroll
            for (int t = 0; t < 4; ++t) zt1[t] = stg_load(st + 4 * g, t);
          }
        }
        // prefetch V^{kk} (input of this layer's tensor product) under the MFMAs that follow
        if (kk > 0) {
          if (!(PARKV && last)) {
#pragma unroll
            for (int lm = 0; lm < 4; ++lm) load_rows<2>(SB, RL + OVIN + 2 * lm, Vk[lm], v16t);
          }
        } else load_rows<4>(SB, R_W0(), W0b, v16t);
        __builtin_amdgcn_sched_barrier(0);
        // down the hidden layers: g_{k-1} = (g_k W_k^T) * silu'(z_{k-1}), then dcat = g_0 W_0^T
        f32x4 dcat[6];
        const int dj = last ? cjump : 0;            // the last layer has no channel mixing: its dcat linear is the one in front of the environment backward
        if constexpr (MD == 1) lin<AR, WT, 6, false, 0>(WB, wp, dh, dcat, v16t, ring, EpiNone{}, dj);
        else {
          f32x4 zt0[WT];
          if constexpr (MD == 3) load_rows<WT>(SB, RL + R_OZ(1, WT), zt0, v16t);
          lin<AR, WT, WT, false, 0>(WB, wp, dh, du, v16t, ring, EpiMulRows<WT>{zt1});
          if constexpr (MD == 3) {
            lin<AR, WT, WT, false, 0>(WB, wp, du, dh, v16t, ring, EpiMulRows<WT>{zt0});
            lin<AR, WT, 6, false, 0>(WB, wp, dh, dcat, v16t, ring, EpiNone{}, dj);
          } else lin<AR, WT, 6, false, 0>(WB, wp, du, dcat, v16t, ring, EpiNone{}, dj);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) dx[t] += dcat[t];
        dVp[0][0] = dcat[4]; dVp[0][1] = dcat[5];             // ds
      }
      if (kk == 0) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          Vk[0][t] = W0b[t];
          Vk[1][t] = W0b[2 + t] * Y1; Vk[2][t] = W0b[2 + t] * Y2; Vk[3][t] = W0b[2 + t] * Y3;
        }
      }
      if (PARKV && last && kk > 0) {                          // the last layer's input tensor, still in the park since its forward pass
#pragma unroll
        for (int lm = 0; lm < 4; ++lm)
#pragma unroll
          for (int t = 0; t < 2; ++t) Vk[lm][t] = park_load(pk, 2 * lm + t, lane);
      }
      f32x4 om1[2];
      load_rows<2>(SB, RL + 2, om1, v16t);                    // omega of this layer, l = 1 part: used after the gradient reduction
      __builtin_amdgcn_sched_barrier(0);
      PHASE(PH_BLAT);
      if (!last) {
        f32x4 in2[2], o2[2];
        in2[0] = park_load(pk, 0, lane); in2[1] = park_load(pk, 1, lane);
        if constexpr (AR == 3) {
          f32x4 i1[2] = {park_load(pk, 2, lane), park_load(pk, 3, lane)}, i2[2] = {park_load(pk, 4, lane), park_load(pk, 5, lane)},
                i3[2] = {park_load(pk, 6, lane), park_load(pk, 7, lane)};
          f32x4 o3[3][2];
          EpiNone ep[3];
          lin_mix(WB, wp, in2, i1, i2, i3, o2, o3, v16t, ring, EpiNone{}, ep, cjump);
          dVp[0][0] += o2[0]; dVp[0][1] += o2[1];
#pragma unroll
          for (int q = 0; q < 3; ++q) { dVp[1 + q][0] = o3[q][0]; dVp[1 + q][1] = o3[q][1]; }
        } else {
          lin<AR, 2, 2, false, 0>(WB, wp, in2, o2, v16t, ring, EpiNone{});
          dVp[0][0] += o2[0]; dVp[0][1] += o2[1];
          in2[0] = park_load(pk, 2, lane); in2[1] = park_load(pk, 3, lane);
          lin<AR, 2, 2, false, 1>(WB, wp, in2, dVp[1], v16t, ring, EpiNone{});
          in2[0] = park_load(pk, 4, lane); in2[1] = park_load(pk, 5, lane);
          lin<AR, 2, 2, false, 2>(WB, wp, in2, dVp[2], v16t, ring, EpiNone{});
          in2[0] = park_load(pk, 6, lane); in2[1] = park_load(pk, 7, lane);
          lin<AR, 2, 2, false, 3>(WB, wp, in2, dVp[3], v16t, ring, EpiNone{});
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      PHASE(PH_BMIX);
      // tensor-product backward: dV (w.r.t. V^{kk}, parked) and the per-edge environment gradient
      {
        const float *en = envrow + kk * (MAXA * ENV_LD);
        const float *tp = lds.tp[kk];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int b = 16 * t + 4 * g;
          const f32x4 e0v = *(const f32x4 *)(en + b), e1v = *(const f32x4 *)(en + 32 + b), e2v = *(const f32x4 *)(en + 64 + b),
                      e3v = *(const f32x4 *)(en + 96 + b);
          const f32x4 v0 = Vk[0][t], v1 = Vk[1][t], v2 = Vk[2][t], v3 = Vk[3][t];
          const f32x4 g0 = dVp[0][t];
          const f32x4 q0 = *(const f32x4 *)(tp + b) * g0, q1 = *(const f32x4 *)(tp + 32 + b) * g0;
          f32x4 a0v = q0 * e0v, a1v = q1 * e1v, a2v = q1 * e2v, a3v = q1 * e3v;       // dV
          f32x4 b0v = q0 * v0, b1v = q1 * v1, b2v = q1 * v2, b3v = q1 * v3;           // denv_e
          if (!last) {
            const f32x4 g1 = dVp[1][t], g2 = dVp[2][t], g3 = dVp[3][t];
            const f32x4 q2 = *(const f32x4 *)(tp + 64 + b), q3 = *(const f32x4 *)(tp + 96 + b), c4 = *(const f32x4 *)(tp + 128 + b);
            const f32x4 q3e0 = q3 * e0v, q2v0 = q2 * v0;
            a0v += q2 * (e1v * g1 + e2v * g2 + e3v * g3);
            b0v += q3 * (v1 * g1 + v2 * g2 + v3 * g3);
            a1v += q3e0 * g1 + c4 * (e2v * g3 - e3v * g2);      // (e x g)_1
            a2v += q3e0 * g2 + c4 * (e3v * g1 - e1v * g3);
            a3v += q3e0 * g3 + c4 * (e1v * g2 - e2v * g1);
            b1v += q2v0 * g1 + c4 * (g2 * v3 - g3 * v2);         // (g x v)_1
            b2v += q2v0 * g2 + c4 * (g3 * v1 - g1 * v3);
            b3v += q2v0 * g3 + c4 * (g1 * v2 - g2 * v1);
          }
          float *sp = st + b;
          *(f32x4 *)(sp) = b0v; *(f32x4 *)(sp + 32) = b1v; *(f32x4 *)(sp + 64) = b2v; *(f32x4 *)(sp + 96) = b3v;
          park_store(pk, 0 + t, a0v, lane);
          park_store(pk, 2 + t, a1v, lane);
          park_store(pk, 4 + t, a2v, lane);
          park_store(pk, 6 + t, a3v, lane);
          __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        reduce_stage(lds, aoffp, lds.denv, na, A.cenv, tid);
        __syncthreads();
      }
      __builtin_amdgcn_sched_barrier(0);
      PHASE(PH_BTP);
      // the saved rows of the next iteration (the layer below, or the embedding), requested in front of this layer's environment backward
      auto next_rows = [&]() __attribute__((always_inline)) {
        if (kk > 0) {                                                      // next iteration's u and z2 rows
          if (!SAVEZ) load_rows<4>(SB, R_LAYER(kk - 1, MD, WT) + OU, upre, v16t);
          load_rows<WT>(SB, R_LAYER(kk - 1, MD, WT) + OZL, zt, v16t);
        } else {                                                           // two-body u and z2 rows, l=1 embedding weights
          if constexpr (!TBT) {
            load_rows<4>(SB, R_U0(), upre, v16t);
            load_rows<4>(SB, R_Z2TB(), zt, v16t);
          } else if constexpr (WT == 4) load_rows<4>(SB, R_Z1TB(), zt, v16t);      // d x0 / dd rows of the two-body table
          else {
#pragma unroll
            for (int t = 0; t < 4; ++t) zt[t] = bload(SB, v16t, (R_Z1TB() + t) * ROW * 4);      // (four rows into the first half of the eight)
          }
          load_rows<2>(SB, R_W0() + 2, w0h, v16t);
        }
      };
      if constexpr (!CEN) {
        f32x4 dom[4];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int b = 16 * t + 4 * g;
          const f32x4 d0 = *(const f32x4 *)(denvrow + b), d1 = *(const f32x4 *)(denvrow + 32 + b), d2 = *(const f32x4 *)(denvrow + 64 + b),
                      d3 = *(const f32x4 *)(denvrow + 96 + b);
          dom[t] = d0;
          dom[2 + t] = d1 * Y1 + d2 * Y2 + d3 * Y3;
          const f32x4 p1 = d1 * om1[t], p2 = d2 * om1[t], p3 = d3 * om1[t];
          dY1 += (p1[0] + p1[1]) + (p1[2] + p1[3]); dY2 += (p2[0] + p2[1]) + (p2[2] + p2[3]); dY3 += (p3[0] + p3[1]) + (p3[2] + p3[3]);
          __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("" : "+v"(dY1), "+v"(dY2), "+v"(dY3));      // summed HERE: sunk to their use at the end of the tile, the sums keep a gradient row alive (in scratch) across the linear below
        next_rows();
        __builtin_amdgcn_sched_barrier(0);
        lin<AR, 4, 4, true, 0>(WB, wp, dom, dx, v16t, ring, EpiNone{});
      } else {
        // The instances with the per-centre form (cen, see the top of the tile).  ONE build of the operand and ONE call site of the linear serve the per-edge form
        // (cen = 0: accumulating into dx) and wave 0's per-centre form (cen = 1: into zeros, which gives P): the operand is  [m0 D0 ; m1 D1 + m2 D2 + m3 D3]  of four rows
        // D of lds.denv either way -- per edge the rows of the lane's centre with m = (1, Y1, Y2, Y3), exactly dom_e; per centre the rows of the column's centre
        // c = j >> 2 with m = the unit vector of its component q = j & 3, or zeros where c >= na.  With a linear in each arm of a branch the ring's registers differ
        // between the arms and the join in front of them copies the in-flight fragments behind s_waitcnt vmcnt(0); with the operand built in each arm,
        // one of its tiles goes to scratch.  The rows of the next iteration are requested in front of every branch here for the same reason.
        // P lives in this layer's environment rows: their last reader, the tensor product above, lies in front of both reduction barriers and their next writer is the
        // next tile's forward reduction; a centre's four 64-vectors at a stride of two rows (2 x 132 >= 4 x 64), so that a lane finds them through envrow.
        float *const pm = lds.env[0] + kk * (MAXA * ENV_LD);
        static_assert(2 * ENV_LD >= 4 * 64 && 3 * 2 * ENV_LD <= Lds<NW>::MAXA * ENV_LD, "the per-centre products of three centres fit a layer's environment rows");
        // what needs only lds.denv and om1: in front of the linear, or, on wave 0 while the others wait for its P, behind the barrier
        auto dy_sums = [&]() __attribute__((always_inline)) {
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const int b = 16 * t + 4 * g;
            const f32x4 p1 = *(const f32x4 *)(denvrow + 32 + b) * om1[t], p2 = *(const f32x4 *)(denvrow + 64 + b) * om1[t], p3 = *(const f32x4 *)(denvrow + 96 + b) * om1[t];
            dY1 += (p1[0] + p1[1]) + (p1[2] + p1[3]); dY2 += (p2[0] + p2[1]) + (p2[2] + p2[3]); dY3 += (p3[0] + p3[1]) + (p3[2] + p3[3]);
          }
          asm volatile("" : "+v"(dY1), "+v"(dY2), "+v"(dY3));
        };
        next_rows();
        if (cen != 1) dy_sums();
        if (cen < 2) {
          const float *dr = denvrow + 4 * g;
          float m0 = 1.f, m1 = Y1, m2 = Y2, m3 = Y3;
          int pcol = 0;
          if (cen == 1) {
            int lq = lane;         // (opaque: the column's addresses are formed here, layer by layer, not once per kernel and held in scratch)
            asm volatile("" : "+v"(lq));
            const int c = (lq >> 2) & 3, q = lq & 3, gq = lq >> 4;
            const bool on = c < na;
            dr = lds.denv + c * ENV_LD + 4 * gq;                 // (c <= 3 < MAXA: a row of the array for every lane)
            m0 = on && q == 0 ? 1.f : 0.f; m1 = on && q == 1 ? 1.f : 0.f; m2 = on && q == 2 ? 1.f : 0.f; m3 = on && q == 3 ? 1.f : 0.f;
            pcol = c < 3 ? c * (2 * ENV_LD) + 64 * q + 4 * gq : -1;       // (the four columns without a centre have no row)
            // wave 0's own gradient waits in its slots of the staging tile (floats 0..63 of a slot's row: idle between the reduction above and the next layer's tensor
            // product, and no other wave touches them): a second accumulator set beside dx costs 16 registers the kernel does not have
#pragma unroll
            for (int t = 0; t < 4; ++t) { *(f32x4 *)(st + 16 * t + 4 * g) = dx[t]; dx[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
          }
          f32x4 dom[4];
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const f32x4 d0 = *(const f32x4 *)(dr + 16 * t), d1 = *(const f32x4 *)(dr + 32 + 16 * t), d2 = *(const f32x4 *)(dr + 64 + 16 * t), d3 = *(const f32x4 *)(dr + 96 + 16 * t);
            dom[t] = d0 * m0;                                    // (per edge: d0 * 1 and d1 Y1 + d2 Y2 + d3 Y3, the values of the per-edge instances)
            dom[2 + t] = d1 * m1 + d2 * m2 + d3 * m3;
          }
          __builtin_amdgcn_sched_barrier(0);
          lin<AR, 4, 4, true, 0>(WB, wp, dom, dx, v16t, ring, EpiNone{});        // the same 16 fragments at the same stream position in both forms
          if (cen == 1) {
            if (pcol >= 0) {
#pragma unroll
              for (int t = 0; t < 4; ++t) *(f32x4 *)(pm + pcol + 16 * t) = dx[t];
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) dx[t] = *(const f32x4 *)(st + 16 * t + 4 * g);
          }
        } else if (cen == 2) {
          wp += lin_frags_h(4, 4) * 256;           // the skipped linear's fragments: the stream jump (cjump) has put the next linear's first RINGH into the ring
          pin_s(wp);
        }
        if (cen) {
          __syncthreads();
          if (cen == 1) dy_sums();
          if (cen != 3) {
            const float *pr = pm + 2 * (envrow - lds.env[0]) + 4 * g;          // = pm + aloc * (2 * ENV_LD)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const f32x4 p0 = *(const f32x4 *)(pr + 16 * t), p1 = *(const f32x4 *)(pr + 64 + 16 * t), p2 = *(const f32x4 *)(pr + 128 + 16 * t),
                          p3 = *(const f32x4 *)(pr + 192 + 16 * t);
              dx[t] += p0 + Y1 * p1 + Y2 * p2 + Y3 * p3;
            }
          }
        }
      }
      PHASE(PH_BENV);
    }
    // ---------------- embedding backward ----------------
    // The NEXT tile's list entries are requested here, two phases before they are used: at the top of a tile they were two dependent
    // round trips (bounds, then entries) behind the wrap-around weight fragments in the in-order return queue -- 8 % of the wave-cycles.
    // Since 4.2c the fetch waits for nothing: its bounds (nb_) were read through the scalar unit at the tile's first barrier.
    tile_fetch(A, nb_, s, tid, nx_);
    // this thread's centre {atom, type}: requested with the next tile's entries, consumed behind the finish barrier.  A range-checked load, not a branch: a branch's join waited for vmcnt(0),
    // i.e. for the acknowledgements of the force atomics below, with the whole workgroup at the barrier behind it.  (Its thread index: an opaque copy, see the finish.)
    int tidc = tid;
    asm volatile("" : "+v"(tidc));
    auto cil_ = __builtin_amdgcn_raw_buffer_load_b64(list_rsrc(A.centre, 8ll * a0, 8 * na), (tidc >> 4) * 8, 0, 0);
    f32x4 zt1b[4];
    if constexpr (!TBT) load_rows<4>(SB, R_Z1TB(), zt1b, v16t);
    __builtin_amdgcn_sched_barrier(0);
    {
      f32x4 dw0[4];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const f32x4 d0 = park_load(pk, 0 + t, lane), d1 = park_load(pk, 2 + t, lane), d2 = park_load(pk, 4 + t, lane), d3 = park_load(pk, 6 + t, lane);
        dw0[t] = d0;
        dw0[2 + t] = d1 * Y1 + d2 * Y2 + d3 * Y3;
#pragma unroll
        for (int r = 0; r < 4; ++r) { dY1 += d1[r] * w0h[t][r]; dY2 += d2[r] * w0h[t][r]; dY3 += d3[r] * w0h[t][r]; }
      }
      asm volatile("" : "+v"(dY1), "+v"(dY2), "+v"(dY3));
      lin<AR, 4, 4, true, 0>(WB, wp, dw0, dx, v16t, ring, EpiNone{});
      if constexpr (TBT) wp = A.o_stream;                                 // last linear of the tile
    }
    PHASE(PH_BEMB);
    // ---------------- two-body embedding backward ----------------
    float dd_part = 0.f;
    if constexpr (TBT) {
      // dE/dd through x0 = sum_f dE/dx0_f * d x0_f / dd (the derivative rows saved by the forward pass, cutoff included)
      f32x4 accv = dx[0] * zt[0];
#pragma unroll
      for (int t = 1; t < 4; ++t) accv += dx[t] * zt[t];
      dd_part = (accv[0] + accv[1]) + (accv[2] + accv[3]);
    } else {
      f32x4 du[4], dh[4];
      float acc = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) { acc += upre[t][r] * dx[t][r]; du[t][r] = fc * dx[t][r]; }
      dfc_part += acc;
      __builtin_amdgcn_sched_barrier(0);
      lin<AR, 4, 4, false, 0>(WB, wp, du, dh, v16t, ring, EpiMulRows<4>{zt});
      lin<AR, 4, 4, false, 0>(WB, wp, dh, du, v16t, ring, EpiMulRows<4>{zt1b});
      f32x4 dbf[2];
      lin<AR, 4, 2, false, 0>(WB, wp, du, dbf, v16t, ring, EpiNone{});   // its prefetches already fetch the next tile's first fragments
      wp = A.o_stream;                                                    // (the stream ends with a copy of its first RING entries)
      const float dfdd = dfc_dx / rc;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float n = (float)(4 * g + r + 1);
        // argument in revolutions for v_sin/v_cos (|arg| <= 4 for the 8 real Bessels): abs error ~1e-6, far
        // inside the force budget; groups 2,3 multiply an exact zero (zero-padded weight columns)
        const float sn = __builtin_amdgcn_sinf(0.5f * n * xx), cs = __builtin_amdgcn_cosf(0.5f * n * xx);
        const float b = pref * sn * inv;
        const float db = pref * (cs * PI * n / rc * inv - sn * inv * inv);
        dd_part += dbf[0][r] * (db * fc + b * dfdd);
      }
    }
    PHASE(PH_BTB);
    // ---------------- geometry backward, outputs ----------------
    {
      const float ibs = AR == 3 ? st[128] : 1.f;
      const float dfc_tot = gsum(dfc_part) * ibs;
      const float dd = dfc_tot * (dfc_dx / rc) + gsum(dd_part) * ibs;
      const float y1 = gsum(dY1) * ibs, y2 = gsum(dY2) * ibs, y3 = gsum(dY3) * ibs;
      const float Gx = C_S3 * y3, Gy = C_S3 * y1, Gz = C_S3 * y2;
      // unit vector and 1 / d again from the edge vector (the same expressions as at the top of the tile): four values less to hold across the whole tile
      float rxe = rx, rye = ry, rze = rz;
      asm volatile("" : "+v"(rxe), "+v"(rye), "+v"(rze));
      const float inve = 1.f / sqrtf(rxe * rxe + rye * rye + rze * rze);
      const float nxe = rxe * inve, nye = rye * inve, nze = rze * inve;
      const float gn = Gx * nxe + Gy * nye + Gz * nze;
      const float gx = dd * nxe + (Gx - gn * nxe) * inve;
      const float gy = dd * nye + (Gy - gn * nye) * inve;
      const float gz = dd * nze + (Gz - gn * nze) * inve;
      if (A.dbg && valid && g == 0) {
        float *dp = A.dbg + 8 * (size_t)e;
        dp[0] = gx; dp[1] = gy; dp[2] = gz; dp[3] = dd; dp[4] = dfc_tot; dp[5] = y1; dp[6] = y2; dp[7] = y3;
      }
#if !defined(ABL_NOW) && !defined(ABL_NOROWS) && !defined(ABL_NOROWLD) && !defined(ABL_NOROWST)
      if (AR == 3 && valid && !(fabsf(gx) + fabsf(gy) + fabsf(gz) + fabsf(eps) < 3.0e38f)) *A.err = 1;      // inf / NaN: an operand left float16's range
#endif
      // The next tile's entries and this thread's centre record are waited for HERE, in front of the force atomics (they were requested a linear ago, nothing younger
      // is in flight): behind the atomics, the first wait for any of them would also wait for the atomics' acknowledgements -- at the top of the next tile.
      asm volatile("" : "+v"(nx_.rx), "+v"(nx_.ry), "+v"(nx_.rz), "+v"(nx_.eii), "+v"(nx_.jat), "+v"(nx_.tt), "+v"(nx_.eoff), "+v"(cil_));
      if (g == 0) {
        st[0] = valid ? gx : 0.f; st[1] = valid ? gy : 0.f; st[2] = valid ? gz : 0.f; st[3] = valid ? eps : 0.f;      // selects, not products: a skipped wave's values are arbitrary
        if (valid) {
#ifndef ABL_NOATOM      // timing experiment only (results are wrong): no force scatter to the neighbour atoms
          atomicAdd(&A.f[3 * (size_t)jat], -(double)gx);
          atomicAdd(&A.f[3 * (size_t)jat + 1], -(double)gy);
          atomicAdd(&A.f[3 * (size_t)jat + 2], -(double)gz);
#endif
        }
      }
      // virial of this wave's 16 edges: butterfly over the slot lanes, lane 0 publishes 6 partials
      float w6[6] = {-rx * gx, -ry * gy, -rz * gz, -0.5f * (rx * gy + ry * gx), -0.5f * (rx * gz + rz * gx), -0.5f * (ry * gz + rz * gy)};
#pragma unroll
      for (int c = 0; c < 6; ++c) w6[c] = valid ? w6[c] : 0.f;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) w6[c] += __shfl_xor(w6[c], off, 64);
      }
      if (lane < 6) {         // after the butterfly every lane holds the 6 totals: lane c owns component c
        const float mine = lane == 0 ? w6[0] : lane == 1 ? w6[1] : lane == 2 ? w6[2] : lane == 3 ? w6[3] : lane == 4 ? w6[4] : w6[5];
        lds.virw[wvq][lq_] += (double)mine;
      }
      if constexpr (VA) vatom_scatter(A.vatom, jat, g, valid, rx, ry, rz, gx, gy, gz);
    }
    // everything the finish derives from the thread index is formed here, from an opaque copy: computed once at kernel entry, those addresses lived
    // the whole tile in scratch and their reloads drained the in-order load queue
    int tidf = tid;
    asm volatile("" : "+v"(tidf));
    const int caf = tidf >> 4;
    __syncthreads();
    const int2 cil = make_int2((int)cil_[0], (int)cil_[1]);
    {
      // per-centre sums of (g, eps): 16 lanes per atom = 4 columns x 4 row-parts; the atom index, scale and
      // shift of this thread's centre were prefetched with the tile.  No trailing barrier: the next tile's first
      // staging write sits behind its own barrier, and its slot offsets go to the other parity buffer.
      const int col = tidf & 3, part = (tidf >> 2) & 3;
      float sum = 0.f;
      if (caf < na)
        for (int sl = aoffp[caf] + part; sl < aoffp[caf + 1]; sl += 4) sum += lds.stage[sl * STG_LD + col];
      sum += __shfl_xor(sum, 4, 64);
      sum += __shfl_xor(sum, 8, 64);
      if (caf < na && part == 0) {
        if (col < 3) atomicAdd(&A.f[3 * (size_t)cil.x + col], (double)sum);
        else {
          const float ei = lds.scale[cil.y] * (sum * A.cenv) + lds.shift[cil.y];
          if (A.eatom) A.eatom[cil.x] = (double)ei;
          lds.eacc[caf] += (double)ei;
        }
      }
    }
    PHASE(PH_FIN);
    if (++ck == A.tchunk) { ck = 0; cpar ^= 1; cbase = __builtin_amdgcn_readfirstlane(lds.chunk[cpar]); }
  }
  __syncthreads();
  int tide = tid;                  // (an opaque copy, as in the finish: what the epilogue derives from the thread index is not kept -- in scratch -- across the tile loop)
  asm volatile("" : "+v"(tide));
  if (tide == 0) {
    for (int a = 0; a < MAXA; ++a) acc_part += lds.eacc[a];
  } else if (tide >= 64 && tide < 70) {
    for (int w = 0; w < NW; ++w) acc_part += lds.virw[w][tide - 64];
  }
  if (PROF && lane == 0) {
#pragma unroll
    for (int k = 0; k < PH_N; ++k) atomicAdd((unsigned long long *)&A.prof[k], (unsigned long long)pacc[k]);
  }
  if (A.prof && tid == 0) {
    // per workgroup: shader cycles, start and end on the constant 100 MHz counter, hardware id (placement)
    long long *o = A.prof + PH_N + 4 * (size_t)blockIdx.x;
    o[0] = clock64() - t_clk0;
    o[1] = t_wall0;
    o[2] = wall_clock64();
    o[3] = ((long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)) << 32) | (unsigned)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));
  }
  if (tide == 0) A.partial[7 * (size_t)blockIdx.x] = acc_part;
  if (tide >= 64 && tide < 70) A.partial[7 * (size_t)blockIdx.x + 1 + (tide - 64)] = acc_part;
}


// ---------------------------------------------------------------------------- the instances, one launch function per part
// (the static_asserts: what a dispatch list names is in fused_shapes.h: FUSED_INSTANCES -- {family, arithmetic, two-body table, MD, RD, WF, RF, option, NW, NL, variant} -- and in this part)
void fused_launch_bf16(int nw, bool prof, int arith, bool tbt, int grid, hipStream_t s, const FusedArgs &A);
void fused_launch_f16(int nw, bool prof, int md, int grid, hipStream_t s, const FusedArgs &A);
void fused_launch_f16_rd2(int nw, int md, int grid, hipStream_t s, const FusedArgs &A);
void fused_launch_f16_w128(int nw, int md, int grid, hipStream_t s, const FusedArgs &A);
void fused_launch_f16_r64(int nw, int md, int grid, hipStream_t s, const FusedArgs &A);
#if AHIP_FUSED_PART == 5
// fused_hq.o: template parameter RT = 4
void fused_launch_f16_r64(int nw, int md, int grid, hipStream_t s, const FusedArgs &A) {
  dispatch<Choices<4, 8>, Choices<1, 2, 3>, Choices<1, 3, 2>, Choices<VAR_VA, VAR_PLAIN>>([&](auto nw, auto nl, auto md, auto var) {
    static_assert(fused_part_holds(AHIP_FUSED_PART, {FusedFamily::k_fused, 3, true, md, 1, 64, 64, false, nw, nl, var}), "not in FUSED_INSTANCES");
    hipLaunchKernelGGL((k_fused<nw, false, 3, true, nl, md, var == VAR_VA, 1, 4, 4>), dim3(grid), dim3(nw * 64), 0, s, A);
  }, nw, A.NL, md, fused_variant(A.vatom, false));
}
#endif
#if AHIP_FUSED_PART == 4
// fused_hm.o: template parameter WT = 8
void fused_launch_f16_w128(int nw, int md, int grid, hipStream_t s, const FusedArgs &A) {
  dispatch<Choices<4, 8>, Choices<1, 2, 3>, Choices<1, 3, 2>, Choices<VAR_VA, VAR_PLAIN>>([&](auto nw, auto nl, auto md, auto var) {
    static_assert(fused_part_holds(AHIP_FUSED_PART, {FusedFamily::k_fused, 3, true, md, 1, 128, 32, false, nw, nl, var}), "not in FUSED_INSTANCES");
    hipLaunchKernelGGL((k_fused<nw, false, 3, true, nl, md, var == VAR_VA, 1, 8>), dim3(grid), dim3(nw * 64), 0, s, A);
  }, nw, A.NL, md, fused_variant(A.vatom, false));
}
#endif
#if AHIP_FUSED_PART == 3
// fused_hr.o: template parameter RD = 2
void fused_launch_f16_rd2(int nw, int md, int grid, hipStream_t s, const FusedArgs &A) {
  dispatch<Choices<4, 8>, Choices<1, 2, 3>, Choices<1, 3, 2>, Choices<VAR_VA, VAR_PLAIN>>([&](auto nw, auto nl, auto md, auto var) {
    static_assert(fused_part_holds(AHIP_FUSED_PART, {FusedFamily::k_fused, 3, true, md, 2, 64, 32, false, nw, nl, var}), "not in FUSED_INSTANCES");
    hipLaunchKernelGGL((k_fused<nw, false, 3, true, nl, md, var == VAR_VA, 2>), dim3(grid), dim3(nw * 64), 0, s, A);
  }, nw, A.NL, md, fused_variant(A.vatom, false));
}
#endif
#if AHIP_FUSED_PART == 2
// fused_h.o
void fused_launch_f16(int nw, bool prof, int md, int grid, hipStream_t s, const FusedArgs &A) {
#ifdef AHIP_ASM_ONLY      // tools/asm_k_fused.sh: the headline instance alone, for a quick look at its code (static census, spills)
#ifndef AHIP_ASM_NW
#define AHIP_ASM_NW 4
#endif
#ifndef AHIP_ASM_NL       // (layers, latent MLP depth, per-atom virial of the instance to look at: AHIP_NL=3 AHIP_MD=1 AHIP_VA=true tools/asm_k_fused.sh)
#define AHIP_ASM_NL 2
#endif
#ifndef AHIP_ASM_MD
#define AHIP_ASM_MD 2
#endif
#ifndef AHIP_ASM_VA
#define AHIP_ASM_VA false
#endif
#ifndef AHIP_ASM_WT       // (AHIP_WT=8: an MLP-width-128 instance; AHIP_RT=4: a read-out-width-64 one)
#define AHIP_ASM_WT 4
#endif
#ifndef AHIP_ASM_RT
#define AHIP_ASM_RT 2
#endif
  hipLaunchKernelGGL((k_fused<AHIP_ASM_NW, false, 3, true, AHIP_ASM_NL, AHIP_ASM_MD, AHIP_ASM_VA, 1, AHIP_ASM_WT, AHIP_ASM_RT>), dim3(grid), dim3(AHIP_ASM_NW * 64), 0, s, A);
#else
  dispatch<Choices<4, 8>, Choices<1, 2, 3>, Choices<1, 3, 2>, Variants>([&](auto nw, auto nl, auto md, auto var) {
    if constexpr (fused_part_holds(AHIP_FUSED_PART, {FusedFamily::k_fused, 3, true, md, 1, 64, 32, false, nw, nl, var}))      // (profiled: one MLP depth only)
      hipLaunchKernelGGL((k_fused<nw, var == VAR_PROF, 3, true, nl, md, var == VAR_VA>), dim3(grid), dim3(nw * 64), 0, s, A);
    else throw StateError("k_fused: not an instance of part 2");
  }, nw, A.NL, md, fused_variant(A.vatom, prof && md == FUSED_PROF_MD));
#endif
}
#endif
#if AHIP_FUSED_PART == 1
// fused_bf.o
void fused_launch_bf16(int nw, bool prof, int arith, bool tbt, int grid, hipStream_t s, const FusedArgs &A) {
  dispatch<Choices<4, 8>, Choices<1, 2>, Choices<1, 0>, Choices<1, 2, 3>, Variants>([&](auto nw, auto b3, auto tb, auto nl, auto var) {
    static_assert(fused_part_holds(AHIP_FUSED_PART, {FusedFamily::k_fused, b3, tb != 0, 2, 1, 64, 32, false, nw, nl, var}), "not in FUSED_INSTANCES");
    hipLaunchKernelGGL((k_fused<nw, var == VAR_PROF, b3, tb != 0, nl, 2, var == VAR_VA>), dim3(grid), dim3(nw * 64), 0, s, A);
  }, nw, arith, tbt, A.NL, fused_variant(A.vatom, prof));
}
#endif

#if AHIP_FUSED_PART == 0
// ---------------------------------------------------------------------------- host side
struct FusedState {
  DevBuf wbuf, scratch;
  TileBufs tiles;
  FusedArgs args;
  bool ready = false, prof_on = false, dbg_on = false, clk_on = false;
  bool tbt = true;             // two-body embedding from the spline table (default) or evaluated as an MLP (option fused_tb=mlp)
  int md = 2;                  // hidden layers of the latent MLP (template parameter MD of k_fused)
  Arith arith = AR_F32;        // arith_policy.h: resolve_arith (every arithmetic has its k_fused instances)
  int part = 0;                // fused_shapes.h: FUSED_INSTANCES
  DevBuf prof, dbg;
  int ncu = 256;
  int force_nw = 0;            // AHIP_FUSED_NW=4|8 pins the workgroup shape (A/B measurements)
};

// bf16x3 fragments of W [K][N]: per (tile pair p, K-step ks) six 1 KiB entries hi0 hi1 mid0 mid1 lo0 lo1; lane (i, g) of an
// entry holds the 8 k-slots of its group: slots 0..3 = rows 16 (2 ks) + 4 g + s, slots 4..7 = rows 16 (2 ks + 1) + 4 g + s - 4;
// column 16 (2 p + half) + i.  Terms by truncation (exact three-way split of the f32 weight).
static inline unsigned bf16_trunc_bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u >> 16; }
static inline float bf16_bits_to_f(unsigned h) { unsigned u = h << 16; float f; std::memcpy(&f, &u, 4); return f; }
static int append_frag_b(std::vector<float> &out, const double *W, int K, int N, int ldw, int nterm = 3) {
  int KS, NT;
  frag_dims_b(K, N, KS, NT);
  for (int p = 0; p < NT / 2; ++p)
    for (int ks = 0; ks < KS; ++ks)
      for (int term = 0; term < nterm; ++term)
        for (int half = 0; half < 2; ++half)
          for (int lane = 0; lane < 64; ++lane)
            for (int w = 0; w < 4; ++w) {
              unsigned word = 0;
              for (int e = 0; e < 2; ++e) {
                const int sl = 2 * w + e, g = lane >> 4;
                const int k = sl < 4 ? 16 * (2 * ks) + 4 * g + sl : 16 * (2 * ks + 1) + 4 * g + (sl - 4);
                const int n = 16 * (2 * p + half) + (lane & 15);
                const float v = (k < K && n < N) ? (float)W[(size_t)k * ldw + n] : 0.f;
                const unsigned hi = bf16_trunc_bits(v);
                const float r1 = v - bf16_bits_to_f(hi);
                const unsigned mid = bf16_trunc_bits(r1);
                const float r2 = r1 - bf16_bits_to_f(mid);
                const unsigned lo = bf16_trunc_bits(r2);
                const unsigned t = term == 0 ? hi : term == 1 ? mid : lo;
                word |= t << (16 * e);
              }
              float f;
              std::memcpy(&f, &word, 4);
              out.push_back(f);
            }
  return 2 * nterm * KS * (NT / 2);
}
// the gate itself: fused_shapes.h
bool fused_model_supported(const Model &m, std::string *why) { return fused_narrow_supported(m.hm, resolve_arith(m, false), fused_tb_is_table(m), why, fused_n_active(m)); }
static_assert(MAXNL == 3, "fused_shapes.h: 1..3 layers");

static void fused_prepare(Model &m) {
  if (!m.fused_state) m.fused_state = new FusedState();
  FusedState &st = *m.fused_state;
  if (st.ready) return;
  const HostModel &h = fused_host_model(m);          // the model at the kernel's fixed widths (zero-padded when it is narrower)
  const int T = h.num_types, NL = h.num_layers;
  std::vector<float> w;
  FusedArgs &A = st.args;
  std::memset(&A, 0, sizeof(A));
  // two-body: pair table (type-type rows of the first layer)
  const int W = h.mlp_width;                      // hidden width of the MLPs at the kernel's shape: 64 or 128 (fused_shapes.h: FUSED_WF, FUSED_WF2)
  const HostTensor &w0 = h.get("tb.w0");          // [2T+8][W]
  A.o_pair = w_mark(w);
  for (int ti = 0; ti < T; ++ti)
    for (int tj = 0; tj < T; ++tj)
      for (int n = 0; n < 64; ++n) w.push_back((float)(w0.data[(size_t)ti * W + n] + w0.data[(size_t)(T + tj) * W + n]));      // (read by fused_tb=mlp only: W = 64)
  // ---- the weight stream, in the order one tile consumes it ----
  A.o_stream = w_mark(w);
  const size_t stream0 = w.size();
  st.tbt = fused_tb_is_table(m);
  st.arith = resolve_arith(m, false);
  st.md = h.mlp_depth;
  const int RF = h.readout_width;                 // read-out width at the kernel's shape: 32 or 64 (fused_shapes.h: FUSED_RF, FUSED_RF2)
  const int MD = st.md, RD = h.readout_depth;
  // the part of this file that holds the model's instances (fused_model_supported keeps a model without one away, fused_host_model pads to a width of the kernels)
  st.part = fused_require_instance({FusedFamily::k_fused, st.arith, st.tbt, MD, RD, W, RF}).part;
  const bool b3 = st.arith == AR_BF16X3 || st.arith == AR_TF32EQ, h2 = st.arith == AR_F16X2, tbt = st.tbt;
  const int nterm = st.arith == AR_BF16X3 ? 3 : 2;
  int h_flags = 0;        // float16 range findings over the weight stream (engine.h: H_RANGE_*)
  auto fwd = [&](const double *W, int K, int N) {
    if (h2) h_flags |= append_frag_h(w, W, K, N, N);
    else if (b3) append_frag_b(w, W, K, N, N, nterm); else append_frag(w, W, K, N, N);
  };
  auto bwd = [&](const double *W, int K, int N) {
    auto t = transpose(W, K, N);
    if (h2) h_flags |= append_frag_h(w, t.data(), N, K, K);
    else if (b3) append_frag_b(w, t.data(), N, K, K, nterm); else append_frag(w, t.data(), N, K, K);
  };
  auto T_ = [&](const std::string &name) -> const double * { return h.get(name).data.data(); };
  const double *wc = w0.data.data() + (size_t)2 * T * W;        // Bessel block [8][W]
  std::vector<double> w3r((size_t)W * RF, 0.0);                 // W3 (last layer, [W][64]) @ Wr (read-out, [64][RF]), float64
  {
    const double *W3 = T_("l" + std::to_string(NL) + ".lat.w" + std::to_string(MD)), *Wr = T_("out.w0");
    for (int i = 0; i < W; ++i)
      for (int q = 0; q < 64; ++q)
        for (int n = 0; n < RF; ++n) w3r[(size_t)i * RF + n] += W3[(size_t)i * 64 + q] * Wr[(size_t)q * RF + n];
  }
  if (!tbt) {
    fwd(wc, 8, 64);
    fwd(T_("tb.w1"), 64, 64);
    fwd(T_("tb.w2"), 64, 64);
  }
  fwd(T_("emb.w"), 64, 64);
  for (int k = 0; k < NL; ++k) {
    const std::string lk = "l" + std::to_string(k + 1);
    fwd(T_(lk + ".env"), 64, 64);
    if (k < NL - 1) {
      const double *mx = T_(lk + ".mix");            // [2][32][32]; the l=1 block serves m = -1, 0, 1
      fwd(mx, 32, 32);
      for (int c = 0; c < (h2 ? 1 : 3); ++c) fwd(mx + 1024, 32, 32);      // f16x2: once, shared by the three components (k_fused: lin_m3)
    }
    fwd(T_(lk + ".lat.w0"), 96, W);
    for (int hl = 1; hl < MD; ++hl) fwd(T_(lk + ".lat.w" + std::to_string(hl)), W, W);
    if (k < NL - 1) fwd(T_(lk + ".lat.w" + std::to_string(MD)), W, 64);
    else {            // last layer: the read-out's first linear applied, multiplied into W3, to z2 and then to x (k_fused, latent MLP)
      fwd(w3r.data(), W, RF);
      fwd(T_("out.w0"), 64, RF);
    }
  }
  if (RD == 2) {      // the read-out's second hidden layer, forward and transposed: two half-ring blocks (k_fused: RD)
    fwd(T_("out.w1"), RF, RF);
    bwd(T_("out.w1"), RF, RF);
  }
  bwd(T_("out.w0"), 64, RF);
  for (int k = NL - 1; k >= 0; --k) {
    const std::string lk = "l" + std::to_string(k + 1);
    if (k < NL - 1) bwd(T_(lk + ".lat.w" + std::to_string(MD)), W, 64);
    else bwd(w3r.data(), W, RF);
    for (int hl = MD - 1; hl >= 1; --hl) bwd(T_(lk + ".lat.w" + std::to_string(hl)), W, W);
    bwd(T_(lk + ".lat.w0"), 96, W);
    if (k < NL - 1) {
      const double *mx = T_(lk + ".mix");
      bwd(mx, 32, 32);
      for (int c = 0; c < (h2 ? 1 : 3); ++c) bwd(mx + 1024, 32, 32);
    }
    bwd(T_(lk + ".env"), 64, 64);
  }
  bwd(T_("emb.w"), 64, 64);
  if (!tbt) {
    bwd(T_("tb.w2"), 64, 64);
    bwd(T_("tb.w1"), 64, 64);
    bwd(wc, 8, 64);
  }
  {   // wrap-around copy: the last linear of a tile prefetches the first fragments of the next tile
    const size_t n = (size_t)(st.arith == AR_BF16X3 ? RINGB : st.arith == AR_TF32EQ ? RINGB2 : h2 ? RINGH : RING) * 256;
    for (size_t i = 0; i < n; ++i) w.push_back(w[stream0 + i]);
  }
  // two-body table (see k_fused), small tables, upload, scalar arguments, float16 range verdict: fused_common.h
  st.ncu = fused_prepare_tail(m, h, w, A, st.wbuf, tbt, 5, 32, nullptr, st.arith, h_flags);
  // Persistent workgroups, 8 waves per CU either way (two per SIMD, 256 registers each).
  A.wave_scratch = (long long)R_TOTAL(NL, MD, W / 16) * ROW;       // (the read-out width does not enter: the RT = 4 instances are f16x2, which save no z (W3 Wr) rows -- and those would fit the layer's four u rows)
  st.scratch.reserve((size_t)st.ncu * 8 * A.wave_scratch * sizeof(float));
  A.scratch = st.scratch.as<float>();
  st.tiles.partial.reserve((size_t)st.ncu * 2 * 7 * sizeof(double));
  if (const char *nwe = std::getenv("AHIP_FUSED_NW")) st.force_nw = std::atoi(nwe);
  st.tiles.ntiles.reserve(64);
  st.prof.reserve((64 + 4 * 2 * (size_t)st.ncu) * sizeof(long long));
  const char *pe = std::getenv("AHIP_FUSED_PROF");
  st.prof_on = pe && pe[0] == '1';
  st.clk_on = std::getenv("AHIP_FUSED_CLK") != nullptr;
  const char *de = std::getenv("AHIP_FUSED_DBG");
  st.dbg_on = de && de[0] == '1';
  st.ready = true;
}

bool fused_run(Model &m, const ComputeArgs &a, std::string *why) {
  // Tile shape (4 waves / 64 slots or 8 waves / 128 slots) follows the largest degree of THIS step's edge list.  The host does not read that
  // back: a degree cannot exceed the row length of the list it was filtered from, which is known since the list was handed
  // over -- rows <= 64: 4 waves, no question; rows <= 128: both shapes are launched and the device word decides (the other kernel returns
  // at once, ~3 us); only lists with longer rows (two-pass edge build, counts read back there) take the decision on the host.
  if (m.edges_T_size != 4) { if (why) *why = "edge vectors are not float32"; return false; }
  fused_prepare(m);
  FusedState &st = *m.fused_state;
  if (st.prof_on || st.clk_on || st.dbg_on) edges_counts(m);      // instrumented runs size their buffers / reports from the counts
  int nw = 0;                                   // 0: decided on the device
  if (!m.counts_pending) {
    if (m.last_max_deg > MAX_TILE_SLOTS) {
      if (why) *why = "an atom has " + std::to_string(m.last_max_deg) + " edges (> 128 per tile)";
      return false;
    }
    nw = m.last_max_deg <= 64 ? 4 : 8;
    if (st.force_nw == 8 || (st.force_nw == 4 && m.last_max_deg <= 64)) nw = st.force_nw;
  } else if (st.force_nw == 8) nw = 8;
  else if (m.max_list_row >= 0 && m.max_list_row <= 64) nw = 4;
  const int *maxdeg_sel = nw == 0 ? m.d_maxdeg : nullptr;
  m.arith.last = st.arith;
  hipStream_t s = a.stream;
  const int tile_slots = nw == 8 ? 128 : 64, maxa = nw == 8 ? Lds<8>::MAXA : Lds<4>::MAXA;      // nw == 0: the packing kernels widen them themselves
  static_assert(Lds<4>::MAXA == FUSED_TILE_MAXA && FUSED_TILE_SLOTS == 64, "allegro_hip.hip requests the 4-wave tile shape from the edge build");
  FusedArgs A = st.args;
  fused_tile_args(m, st.tiles, a, A, tile_slots, maxa, maxdeg_sel, nw == 4);       // (the edge build packs 4-wave tiles only)
  A.maxdeg_sel = maxdeg_sel;
  A.env_bwd = (int)m.opt_env_backward;
  const long long nedges_est = fused_nedges_estimate(m);
  // persistent workgroups fill every CU; reserve_wgs leaves a few slots free so that the exchange kernels of another stream
  // (ghost pack / unpack, RCCL send / recv) can be scheduled while this kernel runs (md.py, overlapped schedule)
  const int grid4 = std::max(1, st.ncu * 2 - m.reserve_wgs), grid8 = std::max(1, st.ncu - m.reserve_wgs);
  const int grid = nw == 8 ? grid8 : grid4;     // rows of `partial` that are summed
  if (nw == 0) AHIP_CHECK(hipMemsetAsync(st.tiles.partial.p, 0, (size_t)grid * 7 * sizeof(double), s));     // the shape that returns at once writes nothing
  {
    StageTimer tm(m, "model_fused", s);
    if (st.dbg_on) {
      st.dbg.reserve((size_t)std::max<long long>(m.nedges, 1) * 8 * sizeof(float));
      AHIP_CHECK(hipMemsetAsync(st.dbg.p, 0, (size_t)m.nedges * 8 * sizeof(float), s));
      A.dbg = st.dbg.as<float>();
    }
    if (st.prof_on || st.clk_on) {
      AHIP_CHECK(hipMemsetAsync(st.prof.p, 0, (64 + 4 * (size_t)grid) * sizeof(long long), s));
      A.prof = st.prof.as<long long>();
    }
    for (int shape = 4; shape <= 8; shape += 4) {
      if (nw != 0 && nw != shape) continue;
      const int g = shape == 8 ? grid8 : grid4;
      A.wg_scratch = shape * A.wave_scratch;
      // claims of TCHUNK tiles amortise the counter's round trip; with few tiles per workgroup the last claim decides the makespan
      // (10 648 Si atoms: 4 659 tiles on 512 workgroups = 12 instead of 10 tile times with claims of 4)
      A.tchunk = (nedges_est / (16 * shape) > (long long)g * 256) ? TCHUNK : 1;
      if (const char *tc = std::getenv("AHIP_TCHUNK")) A.tchunk = std::max(1, std::atoi(tc));       // experiments
      switch (st.part) {
        case 5: fused_launch_f16_r64(shape, st.md, g, s, A); break;
        case 4: fused_launch_f16_w128(shape, st.md, g, s, A); break;
        case 3: fused_launch_f16_rd2(shape, st.md, g, s, A); break;
        case 2: fused_launch_f16(shape, st.prof_on, st.md, g, s, A); break;
        case 1: fused_launch_bf16(shape, st.prof_on, st.arith, st.tbt, g, s, A); break;
        case 0:
          dispatch<Choices<4, 8>, Choices<1, 0>, Choices<1, 2, 3>, Variants>([&](auto nw, auto tb, auto nl, auto var) {
            static_assert(fused_part_holds(AHIP_FUSED_PART, {FusedFamily::k_fused, AR_F32, tb != 0, 2, 1, 64, 32, false, nw, nl, var}), "not in FUSED_INSTANCES");
            hipLaunchKernelGGL((k_fused<nw, var == VAR_PROF, 0, tb != 0, nl, 2, var == VAR_VA>), dim3(g), dim3(nw * 64), 0, s, A);
          }, shape, st.tbt, A.NL, fused_variant(A.vatom, st.prof_on));
          break;
        default: throw StateError("k_fused: no launch function for part " + std::to_string(st.part));
      }
    }
  }
  AHIP_CHECK(hipGetLastError());
  AHIP_CHECK(prim_sum_columns_f64(m.prim, st.tiles.partial.as<double>(), grid, 7, a.engvir, s));
  if (st.prof_on || st.clk_on) {
    std::vector<long long> hp(PH_N + 4 * (size_t)grid);
    AHIP_CHECK(hipMemcpyAsync(hp.data(), st.prof.p, hp.size() * sizeof(long long), hipMemcpyDeviceToHost, s));
    AHIP_CHECK(hipStreamSynchronize(s));
    if (st.prof_on) {
      static const char *names[PH_N] = {"geom", "tb_mlp", "embed", "env+reduce", "tp", "mix", "latent_mlp", "readout", "b_latent", "b_mix", "b_tp+reduce", "b_env", "b_embed", "b_tb", "finish"};
      double tot = 0;
      for (int k = 0; k < PH_N; ++k) tot += (double)hp[k];
      std::fprintf(stderr, "[ahip fused prof] wave-cycles by phase (sum over %d waves):", grid * nw);
      for (int k = 0; k < PH_N; ++k) std::fprintf(stderr, " %s=%.1f%%", names[k], 100.0 * hp[k] / tot);
      std::fprintf(stderr, " | total=%.3g cycles\n", tot);
    }
    {
      // workgroup timeline: spread of start/end times, effective clock, and (AHIP_FUSED_CLK=2) one line per workgroup
      long long t0 = hp[PH_N + 1], t1 = hp[PH_N + 2];
      for (int b = 0; b < grid; ++b) { t0 = std::min(t0, hp[PH_N + 4 * b + 1]); t1 = std::max(t1, hp[PH_N + 4 * b + 2]); }
      double dmin = 1e30, dmax = 0, dsum = 0, smax = 0, mhz = 0;
      for (int b = 0; b < grid; ++b) {
        const long long *o = &hp[PH_N + 4 * b];
        const double d = (double)(o[2] - o[1]) * 1e-5;
        dmin = std::min(dmin, d); dmax = std::max(dmax, d); dsum += d;
        smax = std::max(smax, (double)(o[1] - t0) * 1e-5);
        mhz += (double)o[0] / ((double)(o[2] - o[1]) * 1e-2);
      }
      std::fprintf(stderr, "[ahip fused clk] %d workgroups: kernel span %.3f ms, workgroup duration min/avg/max %.3f/%.3f/%.3f ms, latest start +%.3f ms, %.0f MHz\n",
                   grid, (double)(t1 - t0) * 1e-5, dmin, dsum / grid, dmax, smax, mhz / grid);
      const char *ce = std::getenv("AHIP_FUSED_CLK");
      if (ce && ce[0] == '2')
        for (int b = 0; b < grid; ++b) {
          const long long *o = &hp[PH_N + 4 * b];
          const unsigned hw = (unsigned)o[3], xcc = (unsigned)(o[3] >> 32);
          std::fprintf(stderr, "[ahip fused wg] %d start %.3f end %.3f xcc %u se %u sh %u cu %u\n", b, (double)(o[1] - t0) * 1e-5, (double)(o[2] - t0) * 1e-5,
                       xcc & 15, (hw >> 13) & 7, (hw >> 12) & 1, (hw >> 8) & 15);
        }
    }
  }
  return true;
}

void fused_free(Model &m) {
  if (!m.fused_state) return;
  FusedState *st = m.fused_state;
  for (DevBuf *b : {&st->wbuf, &st->scratch, &st->prof, &st->dbg}) b->release();
  st->tiles.release();
  delete st;
  m.fused_state = nullptr;
}

// ---------------------------------------------------------------------------- diagnostic
// Two-wave self-test of the streamed register-chain linear: out[32][N] = in[32][K] @ W[K][N].
template <int KT, int NT>
__global__ void __launch_bounds__(128) k_selftest_linear(const float *Wf, int wbytes, const float *in, int K, float *out, int N) {
  const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4, row = (threadIdx.x >> 6) * 16 + j;
  f32x4 a[KT], o[NT];
#pragma unroll
  for (int t = 0; t < KT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int k = feat16(t, r, g);
      a[t][r] = k < K ? in[row * K + k] : 0.f;
    }
  __amdgpu_buffer_rsrc_t WB = __builtin_amdgcn_make_buffer_rsrc((void *)Wf, 0, wbytes, 0x00020000);
  f32x4 ring[RING];
  int wp = 0;
  ring_prime(WB, wp, lane * 16, ring);
  linear_s<KT, NT, false, 0>(WB, wp, a, o, lane * 16, ring, EpiNone{});
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int n = feat16(t, r, g);
      if (n < N) out[row * N + n] = o[t][r];
    }
}

template <int KS, int NT, int NTERM>
__global__ void __launch_bounds__(128) k_selftest_linear_b(const float *Wf, int wbytes, const float *in, int K, float *out, int N) {
  const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4, row = (threadIdx.x >> 6) * 16 + j;
  f32x4 a[2 * KS], o[NT];
#pragma unroll
  for (int t = 0; t < 2 * KS; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int k = feat16(t, r, g);
      a[t][r] = k < K ? in[row * K + k] : 0.f;
    }
  Bop b[KS], ob[NT / 2];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) b[ks] = split_pair(a[2 * ks], a[2 * ks + 1]);
  __amdgpu_buffer_rsrc_t WB = __builtin_amdgcn_make_buffer_rsrc((void *)Wf, 0, wbytes, 0x00020000);
  u32x4 ring[RingB<NTERM>::N];
  int wp = 0;
  ring_prime_b(WB, wp, lane * 16, ring);
  linear_b<KS, NT, false, false, 0, EpiNone, NTERM>(WB, wp, b, o, ob, lane * 16, ring, EpiNone{});
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int n = feat16(t, r, g);
      if (n < N) out[row * N + n] = o[t][r];
    }
}

template <int KS, int NT>
__global__ void __launch_bounds__(128) k_selftest_linear_h(const float *Wf, int wbytes, const float *in, int K, float *out, int N) {
  const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4, row = (threadIdx.x >> 6) * 16 + j;
  f32x4 a[2 * KS], o[1][NT];
#pragma unroll
  for (int t = 0; t < 2 * KS; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int k = feat16(t, r, g);
      a[t][r] = k < K ? in[row * K + k] : 0.f;
    }
  Hop b[1][KS], ob[1][NT / 2];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) b[0][ks] = split_pair_h(a[2 * ks], a[2 * ks + 1]);
  __amdgpu_buffer_rsrc_t WB = __builtin_amdgcn_make_buffer_rsrc((void *)Wf, 0, wbytes, 0x00020000);
  u32x4 ring[RINGH];
  int wp = 0;
  ring_prime_b(WB, wp, lane * 16, ring);
  EpiNone ep[1];
  linear_h<1, KS, NT, false, false, 0, EpiNone>(WB, wp, b, o, ob, lane * 16, ring, ep);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int n = feat16(t, r, g);
      if (n < N) out[row * N + n] = o[0][t][r];
    }
}

// The f16x2 operand split alone (fused_h.h: split2_h), pair i = (in[2 i], in[2 i + 1]): out[i] = the packed hi terms, out[npairs + i] = the packed lo' terms.
template <bool MIX> __global__ void __launch_bounds__(256) k_split_probe(const float *in, unsigned *out, int npairs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= npairs) return;
  unsigned h, l;
  split2_h<MIX>(in[2 * i], in[2 * i + 1], h, l);
  out[i] = h;
  out[npairs + i] = l;
}

#endif   // AHIP_FUSED_PART == 0
}  // namespace ahip

#if AHIP_FUSED_PART == 0
using namespace ahip;

// Diagnostic (AHIP_FUSED_DBG=1): per-edge {g[3], dd, dfc, dY[3]} of the last fused compute.
extern "C" int ahip_debug_fused_edges(ahip_model *mh, float *out, long long nedges) {
  ahip::Model *m = (ahip::Model *)mh;
  if (!m || !m->fused_state) return AHIP_ERR_STATE;
  FusedState &st = *m->fused_state;
  if (!st.dbg_on || !st.dbg.p || nedges != m->nedges) return AHIP_ERR_STATE;
  if (hipDeviceSynchronize() != hipSuccess) return AHIP_ERR_DEVICE;
  try { copy_d2h(out, st.dbg.p, (size_t)nedges * 8 * sizeof(float)); } catch (...) { return AHIP_ERR_DEVICE; }
  return 0;
}

extern "C" int ahip_debug_fused_linear(int K, int N, const double *W, const float *in, float *out) {
  try {
    if (const char *sp = std::getenv("AHIP_DEBUG_SPLIT")) {
      // the operand split alone: in[32 K] floats -> out[32 K] words, the 16 K packed hi terms, then the 16 K packed lo' terms; "mix" or "ref" (W is not read)
      const std::string form(sp);
      if (N != K || K < 1 || (form != "mix" && form != "ref")) return AHIP_ERR_UNSUPPORTED;
      const int npairs = 16 * K;
      float *din = nullptr;
      unsigned *dout = nullptr;
      AHIP_CHECK(hipMalloc((void **)&din, (size_t)2 * npairs * sizeof(float)));
      AHIP_CHECK(hipMalloc((void **)&dout, (size_t)2 * npairs * sizeof(unsigned)));
      AHIP_CHECK(hipMemcpy(din, in, (size_t)2 * npairs * sizeof(float), hipMemcpyHostToDevice));
      if (form == "mix") hipLaunchKernelGGL((k_split_probe<true>), dim3((npairs + 255) / 256), dim3(256), 0, 0, din, dout, npairs);
      else hipLaunchKernelGGL((k_split_probe<false>), dim3((npairs + 255) / 256), dim3(256), 0, 0, din, dout, npairs);
      AHIP_CHECK(hipDeviceSynchronize());
      AHIP_CHECK(hipMemcpy(out, dout, (size_t)2 * npairs * sizeof(unsigned), hipMemcpyDeviceToHost));
      (void)hipFree(din); (void)hipFree(dout);
      return 0;
    }
    const char *ar = std::getenv("AHIP_FUSED_ARITH");
    const int nterm = (ar && std::string(ar) == "tf32eq") ? 2 : 3;
    const bool h2 = ar && std::string(ar) == "f16x2";
    const bool b3 = h2 || (ar && (std::string(ar) == "b3" || std::string(ar) == "bf16x3" || std::string(ar) == "tf32eq"));
    std::vector<float> frag;
    int KT, NT;
    if (h2) { append_frag_h(frag, W, K, N, N); frag_dims_b(K, N, KT, NT); }
    else if (b3) { append_frag_b(frag, W, K, N, N, nterm); frag_dims_b(K, N, KT, NT); }
    else { append_frag(frag, W, K, N, N); frag_dims(K, N, KT, NT); }
    frag.resize(frag.size() + (size_t)(RINGB + 2) * 256, 0.f);      // the ring prefetches past the end
    float *dW = nullptr, *din = nullptr, *dout = nullptr;
    AHIP_CHECK(hipMalloc((void **)&dW, frag.size() * sizeof(float)));
    AHIP_CHECK(hipMalloc((void **)&din, (size_t)32 * K * sizeof(float)));
    AHIP_CHECK(hipMalloc((void **)&dout, (size_t)32 * N * sizeof(float)));
    AHIP_CHECK(hipMemcpy(dW, frag.data(), frag.size() * sizeof(float), hipMemcpyHostToDevice));
    AHIP_CHECK(hipMemcpy(din, in, (size_t)32 * K * sizeof(float), hipMemcpyHostToDevice));
    bool ok = true;
    const int wbytes = (int)(frag.size() * sizeof(float));
#define CASEB(ks, nt) do { if (h2) hipLaunchKernelGGL((k_selftest_linear_h<ks, nt>), dim3(1), dim3(128), 0, 0, dW, wbytes, din, K, dout, N); \
                           else if (nterm == 3) hipLaunchKernelGGL((k_selftest_linear_b<ks, nt, 3>), dim3(1), dim3(128), 0, 0, dW, wbytes, din, K, dout, N); \
                           else hipLaunchKernelGGL((k_selftest_linear_b<ks, nt, 2>), dim3(1), dim3(128), 0, 0, dW, wbytes, din, K, dout, N); } while (0)
#define CASEH(ks, nt) hipLaunchKernelGGL((k_selftest_linear_h<ks, nt>), dim3(1), dim3(128), 0, 0, dW, wbytes, din, K, dout, N)
    if (b3) {
      if (KT == 1 && NT == 2) CASEB(1, 2);
      else if (KT == 1 && NT == 4) CASEB(1, 4);
      else if (KT == 2 && NT == 2) CASEB(2, 2);
      else if (KT == 2 && NT == 4) CASEB(2, 4);
      else if (KT == 3 && NT == 4) CASEB(3, 4);
      else if (KT == 2 && NT == 6) CASEB(2, 6);
      // the f16x2 shapes of the MLP-width-128 instances (k_fused WT = 8, k_fused_lx HT = 8)
      else if (h2 && KT == 3 && NT == 8) CASEH(3, 8);
      else if (h2 && KT == 4 && NT == 8) CASEH(4, 8);
      else if (h2 && KT == 4 && NT == 4) CASEH(4, 4);
      else if (h2 && KT == 1 && NT == 8) CASEH(1, 8);
      else if (h2 && KT == 4 && NT == 6) CASEH(4, 6);
      else if (h2 && KT == 2 && NT == 8) CASEH(2, 8);
      else if (h2 && KT == 4 && NT == 2) CASEH(4, 2);
      else ok = false;
    } else
#undef CASEB_
#undef CASEH
#define CASE(kt, nt) hipLaunchKernelGGL((k_selftest_linear<kt, nt>), dim3(1), dim3(128), 0, 0, dW, wbytes, din, K, dout, N)
    if (KT == 2 && NT == 2) CASE(2, 2);
    else if (KT == 2 && NT == 4) CASE(2, 4);
    else if (KT == 4 && NT == 2) CASE(4, 2);
    else if (KT == 4 && NT == 4) CASE(4, 4);
    else if (KT == 6 && NT == 4) CASE(6, 4);
    else if (KT == 4 && NT == 6) CASE(4, 6);
    else ok = false;
#undef CASE
    if (ok) {
      AHIP_CHECK(hipDeviceSynchronize());
      AHIP_CHECK(hipMemcpy(out, dout, (size_t)32 * N * sizeof(float), hipMemcpyDeviceToHost));
    }
    (void)hipFree(dW); (void)hipFree(din); (void)hipFree(dout);
    return ok ? 0 : AHIP_ERR_UNSUPPORTED;
  } catch (const std::exception &) { return AHIP_ERR_DEVICE; }
}
#endif   // AHIP_FUSED_PART == 0

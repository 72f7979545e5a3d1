// Fused MFMA path for the wider Allegro shape l_max = 2 with 32 tensor features (the reference test YAML's shape: l_max = 2, U = 32, 3 layers,
// /root/reference/tests/test_data/test_repro_allegro.yaml:89-99; 64 tensor features, BASELINE config 5's model L, run on k_fused_lx2, fused_lx2.hip).  Same mapping as fused.hip (one launch = forward + analytic
// backward, every per-edge vector in the v_mfma_f32_16x16x4_f32 C/D layout, weights as one A-fragment stream in consumption
// order, per-centre reductions through LDS, saved rows in a per-wave scratch) with what the larger state forces:
//
//  * The edge tensor V[lm][u] is D*U = 576 floats per edge for model L: 144 registers per lane.  It stays in REGISTERS for the
//    whole tile -- streaming it through memory would cost ~50 KB per edge per step -- so a wave owns the whole 512-entry
//    register file of its SIMD: one 4-wave workgroup (64 edge slots) per CU, __launch_bounds__(256, 1).
//  * The tensor product is channel-wise, so it runs one 16-feature K-tile t at a time IN PLACE on V[.][t] (9 + 9 live rows), with
//    the Clebsch-Gordan table unrolled at compile time from cg_tables.h; the channel mixing V[lm] <- V[lm] @ M_l is done in place
//    per (l, m) row; backward the same way (mix^T in place, then the tensor-product gradient in place per K-tile).
//  * The per-centre environment sum goes through a double-buffered LDS stage holding ONE K-tile ([slots][D x 16]); one barrier
//    per K-tile.
//  * Two-body embedding from the per-type-pair spline table (fused_common.h), always.
// Reference graph: the TorchScript model executed at /root/reference/pair_nequip_allegro.cpp:409-430; the oracle is
// oracle/allegro_torch.py (autograd), so the hand-derived backward below is checked against an independent derivation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/allegro_hip.h"
#ifndef AHIP_ROW_AUX
#define AHIP_ROW_AUX 2          // saved rows: non-temporal (fused_common.h)
#endif
#include "engine.h"
#include "fused_lx_common.h"
#include "prims.h"

namespace ahip {

// The shape of k_fused_lx: l_max = 2, 2 16-feature tiles (32 tensor features); NW = 4 waves (one per SIMD, 64 edge slots) or 8 (two per SIMD, 128 slots:
// centres with 65..128 edges, option wide_tile=auto); HT = 16-feature tiles of a hidden layer of the latent MLP: 4 (MLP width <= 64) or 8 (65..128, zero-padded to 128),
// which only the saved-row map knows (the read-out's tile count, template parameter RT of the kernel, touches neither the shape nor the rows)
template <int NW_, int HT_ = 4> struct ShapeX {
  static_assert(NW_ == 4 || NW_ == 8, "4- or 8-wave tiles");
  static_assert(HT_ == 4 || HT_ == 8, "hidden layers of 64 or 128 features");
  static constexpr int L = 2, UT = 2, NW = NW_;
  static constexpr int D = (L + 1) * (L + 1), NLP = L + 1, U = 16 * UT, EW = NLP * UT;   // EW: 16-feature tiles of an (l, u) weight vector
  static constexpr int SLOTS = 16 * NW;
  static constexpr int MAXA = lx_tile_maxa(NW == 8);    // centre atoms per tile: 4 / 8 (LDS budget of the environment rows; fused_shapes.h)
  static_assert(SLOTS == lx_tile_slots(NW == 8), "fused_shapes.h: the tile shapes the dispatch asks the packing for");
  static constexpr int STG_LD = D * 16 + 4;             // one K-tile of a slot: [lm][16] + pad (16-byte rows, conflict-free b128 writes)
  static constexpr int ENVA = D * U + 4;                // environment row of one centre: [lm][u] + pad
  static constexpr int NP = CgX<L>::NP;
  // scratch rows (per wave, 1 KiB each): d x0/dd 4 | w0 EW | per layer: omega EW, hidden layers 1..MD HT each, u 4, V_in D*UT  (fused_lx_rows.h; MD = latent MLP depth)
  using R = std::conditional_t<HT_ == 4, RowsX, RowsXM>;
  static_assert(R::EW == EW && R::NV == D * UT && R::HR == HT_ && R::UR == 4, "row map of this shape");
  static constexpr int R_DX0 = R::R_DX0, R_W0 = R::R_W0, O_OM = R::O_OM;
  __host__ __device__ static constexpr int O_Z(int h) { return R::O_Z(h); }
  __host__ __device__ static constexpr int O_U(int MD) { return R::O_U(MD); }
  __host__ __device__ static constexpr int O_VIN(int MD) { return R::O_VIN(MD); }
  __host__ __device__ static constexpr int LSZ(int MD) { return R::LSZ(MD); }
  __host__ __device__ static constexpr int R_LAYER(int kk, int MD) { return R::R_LAYER(kk, MD); }
  __host__ __device__ static constexpr int R_TOTAL(int NL, int MD) { return R::R_TOTAL(NL, MD); }
};

template <int NW_> struct __attribute__((aligned(16))) LdsX {
  using S = ShapeX<NW_>;
  static constexpr int NW = S::NW;
  // 4 waves: double-buffered (one barrier per K-tile).  8 waves: two buffers of 128 slots alone would be 151 KB, so ONE, and a second barrier per K-tile
  // (every wave has read K-tile t before t + 1 is written) that the other wave of the SIMD covers
  static constexpr int NSTG = NW == 4 ? 2 : 1;
  float stage[NSTG][S::SLOTS * S::STG_LD];
  float env[LX_MAXNL][S::MAXA * S::ENVA];
  float denv[S::MAXA * S::ENVA];
  float tp[LX_MAXNL][S::NP * S::U];          // tensor-product path weights [layer][path][u]
  double eacc[S::MAXA];
  double virw[NW][6];
  int aoff[2][S::MAXA + 2];
  float rc[256];                             // model cutoff table [T*T], T <= 16 (the edge build packs a type in 4 bits)
  float scale[16], shift[16];
  float res[LX_MAXNL][2];
  int chunk[2];
  // Round 6: rows of the LAST layer that never travel to memory.  One workgroup per CU leaves ~58 KB of LDS unused: per wave NLROW register-image rows hold the last
  // layer's omega rows (l >= 1) and the first rows of its input tensor; its 8 latent-MLP rows go to the wave's own slots of stage[0], idle between that layer's
  // environment sum and its backward tensor product (as in k_fused: EpiSiluSaveDL / EpiSiluSaveZL).  22 of the 118 rows a wave-tile of the reference YAML's shape saves.
  // 8 waves (one workgroup per CU again, 128-slot stage, 8 centres): room for the last layer's 4 omega rows only -- its input tensor rows all go to the wave's scratch
  // like a non-last layer's (NVL = 0 in the kernel).  stage 74 KB + env / denv 36.5 KB + tp 5.6 KB + rowsl 32 KB + tables = 153 392 B
  static constexpr int NLROW = NW == 4 ? 14 : 4;
  float rowsl[NW][NLROW * ROW];
};
static_assert(sizeof(LdsX<4>) <= 160 * 1024 && sizeof(LdsX<8>) <= 160 * 1024, "LDS budget of one CU");


// Per-centre sum of one staged K-tile: env[a][lm][16 t + f] = scale * sum_{slots of a} stage[slot][lm][f].
// Work item = (centre, 4-feature column); its LPI adjacent lanes take every LPI-th slot with 16-byte LDS reads (all of a lane's reads
// are in flight together) and combine with log2(LPI) cross-lane adds -- a fixed order, so the sums are reproducible.
template <int NW>
__device__ __forceinline__ void reduce_stage_x(const float *stg, const int *aoff, float *dst, int na, float scale, int t, int uwave) {
  using S = ShapeX<NW>;
  constexpr int LPI = 4;                    // lanes per work item: 36 columns x 4 lanes = one round for a tile that holds one centre
  constexpr int NC = S::D * 4, PER_ROUND = NW * 64 / LPI, NRD = S::SLOTS / LPI;
  // lane -> (item, part): part = lane / 16, item = 16 * wave + lane % 16.  The 16 lanes of one 16-byte LDS read phase then hold 16
  // consecutive 4-feature columns of the same slot: distinct banks.  (Adjacent lanes = the parts of one item hit rows 148 floats
  // apart with 16-byte reads: SQ_LDS_BANK_CONFLICT was 76 % of the LDS-active cycles.)
  static_assert(LPI == 4, "four 16-lane groups");
  const int lane = fresh_lane();
  const int p = lane >> 4;
  for (int it = uwave * 16 + (lane & 15); it < ((na * NC + PER_ROUND - 1) / PER_ROUND) * PER_ROUND; it += PER_ROUND) {   // whole waves iterate together
    const bool live = it < na * NC;
    const int a = live ? it / NC : 0, c = live ? it - a * NC : 0;
    const int s0 = aoff[a] + p, s1 = live ? aoff[a + 1] : 0;
    // all reads are issued before the first is used: addresses past the centre's last slot are clamped to slot 0 of the stage
    // (always mapped) and their values discarded -- a conditional read per slot costs one LDS round trip each
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (NW == 4) {
      f32x4 v[NRD];
#pragma unroll
      for (int k = 0; k < NRD; ++k) {
        const int sl = s0 + LPI * k;
        v[k] = *(const f32x4 *)(stg + (sl < s1 ? sl : 0) * S::STG_LD + 4 * c);
      }
#pragma unroll
      for (int k = 0; k < NRD; ++k)
        if ((s0 + LPI * k) < s1) acc += v[k];
    } else {
      // 8 waves: 32 reads per lane, in batches of 8 -- the edge tensor sits in ordinary registers there and 128 more would all be spilled
      constexpr int NB = 8;
#pragma unroll
      for (int k0 = 0; k0 < NRD; k0 += NB) {
        f32x4 v[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          const int sl = s0 + LPI * (k0 + k);
          v[k] = *(const f32x4 *)(stg + (sl < s1 ? sl : 0) * S::STG_LD + 4 * c);
        }
#pragma unroll
        for (int k = 0; k < NB; ++k)
          if ((s0 + LPI * (k0 + k)) < s1) acc += v[k];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v1 = acc[r];
      v1 += __shfl_xor(v1, 16, 64);
      v1 += __shfl_xor(v1, 32, 64);
      acc[r] = v1 * scale;
    }
    if (live && p == 0) *(f32x4 *)(dst + a * S::ENVA + (c >> 2) * S::U + 16 * t + 4 * (c & 3)) = acc;
  }
}

// Channel mixing, one (l, m) row at a time, in place on the parked edge tensor: V[lm] <- V[lm] @ M_l (forward, output rows
// saved as the next layer's V_in) or V[lm] <- V[lm] @ M_l^T (+ ds on the scalar row: backward).  With 32 tensor features a row
// is 2 x 2 tiles = 4 weight fragments = half a ring: rows alternate the ring phase, and the last (ninth) row is zero-padded on
// the host to 8 fragments so that the stream stays ring-aligned.
template <int LM, int D, int UT, bool FWD, int AR, bool LSPLIT = false>
__device__ __forceinline__ void mix_rows(float (&V)[D][UT][4], __amdgpu_buffer_rsrc_t WB, int &wp, int v16, LxRing<AR> &ring,
                                         __amdgpu_buffer_rsrc_t SB, int row0, const f32x4 (&ds)[UT], float *lbase = nullptr, int lrow0 = 0, int nlds = 0) {
  if constexpr (LM < D) {
    constexpr bool PADDED = (UT == 2) && (LM == D - 1) && (D % 2 == 1);
    constexpr int NTO = PADDED ? 4 : UT;
    constexpr int RP = (UT == 2 && !PADDED) ? 4 * (LM & 1) : 0;
    f32x4 vi[UT], o[NTO];
#pragma unroll
    for (int t = 0; t < UT; ++t) vi[t] = acc_get4(V[LM][t]);
    v16 = fresh_lane() << 4;          // formed here (as fused_lx2.hip does): the value computed at kernel entry was spilled and reloaded in front of every row store
    if constexpr (FWD) {
      // (lbase: the output rows are the LAST layer's input tensor -- its first nlds rows stay in LDS)
      if constexpr (LSPLIT) lx_lin<AR, UT, NTO, false, RP>(WB, wp, vi, o, v16, ring, EpiSaveNSplit<UT>{SB, row0, v16, lbase, LM * UT, lrow0, nlds, fresh_lane()});
      else lx_lin<AR, UT, NTO, false, RP>(WB, wp, vi, o, v16, ring, EpiSaveN<UT>{SB, row0 + LM * UT, v16});
    } else lx_lin<AR, UT, NTO, false, RP>(WB, wp, vi, o, v16, ring, EpiNone{});
#pragma unroll
    for (int t = 0; t < UT; ++t) acc_put4(V[LM][t], (!FWD && LM == 0) ? o[t] + ds[t] : o[t]);
    __builtin_amdgcn_sched_barrier(0);
    mix_rows<LM + 1, D, UT, FWD, AR, LSPLIT>(V, WB, wp, v16, ring, SB, row0, ds, lbase, lrow0, nlds);
  }
}

enum { PX_GEOM = 0, PX_EMB, PX_ENV, PX_TP, PX_LAT, PX_MIX, PX_OUT, PX_BLAT, PX_BMIX, PX_BTP, PX_BENV, PX_BEMB, PX_FIN, PX_N };
#define PHASEX(id) do { if (PROF) { long long _t = clock64(); pacc[id] += _t - tprev; tprev = _t; } } while (0)

// ---------------------------------------------------------------------------- the kernel
// NLT = number of layers: the layer loops are unrolled so that `last layer` / `first layer` are compile-time facts -- with
// run-time branches inside them the register allocator shuffles dozens of spill slots at every join (load, wait, store).
// VA: also the per-atom virial (output "atomic_virial": fused_common.h, vatom_scatter); launched only while that output is registered
// MD: hidden layers of the latent MLP (allegro_mlp_hidden_layers_depth; 2 in the reference test YAML).  1 and 3 exist on the f16x2 arithmetic only, as in k_fused;
// every MD-dependent piece below is `if constexpr`, and the MD = 2 instances are what they were before the parameter existed.  RD: hidden layers of the read-out MLP (1; 2 on f16x2 only, built in fused_lx_r.o).
// NW: waves per workgroup = 16-slot groups of a tile.  4: one wave per SIMD, the edge tensor parked in AGPRs.  8: two waves per SIMD, 256 registers each, no park
// (compiled with AHIP_NO_ACC_PARK in an object of its own: fused_lx_w.o), one staging buffer; (MD, RD) = (2, 1), not profiled.
// HT: 16-feature tiles of one hidden layer of the latent MLP: 4, or 8 for MLP width 65..128 zero-padded to 128 (f16x2, 4-wave tiles, read-out depth 1, not profiled; built in
// fused_lx_m.o).  Only the hidden vectors and their saved rows grow (as in k_fused: template parameter WT); the LDS is that of HT = 4.  RT: 16-feature tiles of the read-out MLP's hidden layer: 2, or 4 for read-out width 33..64 zero-padded to 64 (f16x2, 4-wave tiles, HT = 4, read-out depth 1, not profiled; built in fused_lx_q.o).  Only the read-out vectors of the tile grow: the read-out saves no rows, so row map, scratch and LDS are those of RT = 2.
template <int NW, int NLT, bool PROF, int AR, bool VA = false, int MD = 2, int RD = 1, int HT = 4, int RT = 2>
__global__ void __launch_bounds__(NW * 64, 1) k_fused_lx(FusedLxArgs A) {
  using S = ShapeX<NW, HT>;
  using LdsT = LdsX<NW>;
  constexpr int L = S::L, UT = S::UT;
  static_assert(NW == 4 || (MD == 2 && RD == 1 && !PROF), "8-wave tiles: MLP depth 2, read-out depth 1, not profiled");
  constexpr int NTHREADS = NW * 64, D = S::D, U = S::U, EW = S::EW, MAXA = S::MAXA, STG_LD = S::STG_LD, ENVA = S::ENVA, NP = S::NP;
  constexpr bool SAVEZ = AR == 3;          // f16x2: raw pre-activation rows of the last hidden layer instead of silu' rows, no u rows (see fused.hip)
  static_assert(MD >= 1 && MD <= 3 && (MD == 2 || AR == 3), "latent MLP depth 1 / 3: f16x2 instances only");
  static_assert(MD == 2 || !PROF, "profiled instances: depth 2");
  static_assert(RD == 1 || (RD == 2 && AR == 3 && !PROF), "read-out depth 2: f16x2 instances only, not profiled");
  // The last model layer keeps its latent-MLP rows in the staging tile: the last hidden layer in images ZIMG .. ZIMG + 3, the one below it (MD >= 2) in images 0..3.
  // A wave's slots hold 9 images; depth 3 would need 12, so the silu' rows of its hidden layer 1 go to the per-wave scratch like a non-last layer's.
  // HT = 8: the 8 images of the last hidden layer fill the slot (images 0..7 of 9); every hidden layer below it goes to the scratch rows, in the last model layer too.
  constexpr int ZIMG = (MD == 1 || HT == 8) ? 0 : 4;
  static_assert(HT == 4 || (HT == 8 && NW == 4 && AR == 3 && RD == 1 && !PROF), "MLP width 128: f16x2 instances on 4-wave tiles, read-out depth 1, not profiled");
  static_assert(HT <= D, "the last hidden layer's images fit a staging slot");
  static_assert(RT == 2 || (RT == 4 && NW == 4 && AR == 3 && RD == 1 && HT == 4 && !PROF), "read-out width 64: f16x2 instances on 4-wave tiles, MLP width 64, read-out depth 1, not profiled");
  static_assert(lin_frags_h(4, RT) % RINGH == 0 && lin_frags_h(RT, 4) % RINGH == 0, "the weight ring stays in phase");
  // every linear whose shape depends on HT consumes whole rings of the weight stream: the ring phases of the mixing rows are those of HT = 4
  static_assert(lin_frags_h(4 + UT, HT) % RINGH == 0 && lin_frags_h(HT, HT) % RINGH == 0 && lin_frags_h(HT, 4) % RINGH == 0 && lin_frags_h(4, HT) % RINGH == 0 &&
                    lin_frags_h(HT, 4 + UT) % RINGH == 0, "the weight ring stays in phase");
  // last-layer rows in LDS (LdsX::rowsl, stage[0] images): LDS rows [0, NOML) = omega l >= 1, [NOML, NLROW) = the first NVL rows of the input tensor
  constexpr int NLROW = LdsT::NLROW, NSTG = LdsT::NSTG, NOML = L * UT, NVL = (NLROW - NOML) < D * UT ? (NLROW - NOML) : D * UT;
  static_assert(NOML <= NLROW, "omega rows of the last layer fit the LDS rows");
  __shared__ LdsT lds;
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 15, g = lane >> 4, wave = tid >> 6;
  const int uwave = __builtin_amdgcn_readfirstlane(wave);
  const int v16 = lane * 16;
  __amdgpu_buffer_rsrc_t SB, WB;
  {
    unsigned long long b = (unsigned long long)(A.scratch + (size_t)blockIdx.x * A.wg_scratch + (size_t)wave * A.wave_scratch);
    unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    SB = __builtin_amdgcn_make_buffer_rsrc((void *)(((unsigned long long)hi << 32) | lo), 0, (int)(A.wave_scratch * 4), 0x00020000);
    WB = __builtin_amdgcn_make_buffer_rsrc((void *)A.wbase, 0, A.wbytes, 0x00020000);
  }
  const float *__restrict__ Wb = A.wbase;
  constexpr int NL = NLT;
  for (int k = tid; k < NL * NP * U; k += NTHREADS) lds.tp[k / (NP * U)][k % (NP * U)] = Wb[A.o_tpl + k];
  const int ntiles = *A.ntiles;
  double acc_part = 0.0;
  long long pacc[PX_N];
  long long tprev = 0;
  if (PROF) {
#pragma unroll
    for (int k = 0; k < PX_N; ++k) pacc[k] = 0;
    tprev = clock64();
  }
  LxRing<AR> ring;
  int wp = A.o_stream;
  lx_prime<AR>(WB, wp, v16, ring);
  if (tid < MAXA) lds.eacc[tid] = 0.0;
  if (lane < 6) lds.virw[wave][lane] = 0.0;
  if (tid < A.T * A.T) lds.rc[tid] = (float)A.rcut[tid];
  if (tid < A.T) { lds.scale[tid] = Wb[A.o_scale + tid]; lds.shift[tid] = Wb[A.o_shift + tid]; }
  if (tid < 2 * NL) lds.res[tid >> 1][tid & 1] = Wb[A.o_res[tid >> 1] + (tid & 1)];

  const int s = wave * 16 + j;                 // this lane's edge slot
  const int ca = tid >> 4;                     // centre slot served by this thread in the per-centre output step
  if (tid == 0) lds.chunk[0] = (int)atomicAdd(A.tile_counter, (unsigned)A.tchunk);
  __syncthreads();
  int par = 0, cpar = 0, ck = 0;
  int cbase = __builtin_amdgcn_readfirstlane(lds.chunk[0]);

  for (;;) {
    const int tile = cbase + ck;
    if (tile >= ntiles) break;
    int claimed = 0;
    if (ck == 0 && tid == 0) claimed = (int)atomicAdd(A.tile_counter, (unsigned)A.tchunk);
    const int a0 = A.tile_a0[tile], a1 = A.tile_a0[tile + 1], e0 = A.tile_e0[tile], e1 = A.tile_e0[tile + 1];
    const int na = a1 - a0;
    if (e1 - e0 > S::SLOTS) {
      // a single centre with more edges than the tile has slots (the packing gives such a centre a tile of its own): it is
      // evaluated by the layer-at-a-time kernels afterwards (heavy_generic, allegro_hip.hip)
      if (ck == 0 && tid == 0) lds.chunk[cpar ^ 1] = claimed;
      __syncthreads();
      if (++ck == A.tchunk) { ck = 0; cpar ^= 1; cbase = __builtin_amdgcn_readfirstlane(lds.chunk[cpar]); }
      continue;
    }
    par ^= 1;
    int *const aoffp = lds.aoff[par];
    const int e = e0 + s;
    const bool valid = e < e1;
    float rx = 1.f, ry = 0.f, rz = 0.f;
    int aloc = 0, ti = 0, tj = 0, jat = 0, c_i = 0, c_t = 0;
    if (valid) {
      rx = A.rvec[3 * (size_t)e]; ry = A.rvec[3 * (size_t)e + 1]; rz = A.rvec[3 * (size_t)e + 2];
      aloc = A.e_ii[e] - a0;
      jat = A.e_j[e];
      const int tt = A.e_tt[e];
      ti = tt >> 4; tj = tt & 15;
    }
    if (ca < na) { const int2 ci = A.centre[a0 + ca]; c_i = ci.x; c_t = ci.y; }
    if (tid <= na) aoffp[tid] = A.eoff[a0 + tid] - e0;

    // ---------------- geometry ----------------
    const float d = sqrtf(rx * rx + ry * ry + rz * rz);
    const float inv = 1.f / d;
    const float nx = rx * inv, ny = ry * inv, nz = rz * inv;
    const float rc = lds.rc[ti * A.T + tj];
    const float xx = d / rc;
    float fc, dfc_dx;
    cutoff_poly_c(A.p, A.cp, xx, fc, dfc_dx);
    if (!valid) { fc = 0.f; dfc_dx = 0.f; }
    // real spherical harmonics, component normalisation, m = -l..l (pair_allegro_amd/cg.py)
    constexpr float C3 = 1.7320508075688772f, C15 = 3.872983346207417f, C5H = 1.118033988749895f;
    float Y[D];
    Y[0] = 1.f;
    Y[1] = C3 * ny; Y[2] = C3 * nz; Y[3] = C3 * nx;
    if constexpr (L >= 2) {
      Y[4] = C15 * nx * ny; Y[5] = C15 * ny * nz; Y[6] = C5H * (2.f * nz * nz - nx * nx - ny * ny);
      Y[7] = C15 * nx * nz; Y[8] = 0.5f * C15 * (nx * nx - ny * ny);
    }
    const int envoff = aloc * ENVA + 4 * g;      // + kk * MAXA*ENVA (layer) + lm * U + 16 t
    // this lane's staging row in buffer b, formed where it is used from the hardware lane counter (round 6): as a value computed at the top of the tile it
    // lived in scratch once the last layer's rows moved into the stage, and its reload in front of every staging write drained the in-order load queue
    auto STQ = [&](int b) { const int ln = fresh_lane(); return lds.stage[NSTG == 2 ? b : 0] + (uwave * 16 + (ln & 15)) * STG_LD + 4 * (ln >> 4); };
    PHASEX(PX_GEOM);

    // ---------------- two-body embedding x0(d; type pair) from the spline table ----------------
    f32x4 x[4];
    {
      lx_prime<AR>(WB, wp, v16, ring);        // RING_DROP: not carried through the finish / geometry phases of the tile boundary either
      const float tb_invh = (float)A.tb_nk / rc;
      const float sft = d * tb_invh;
      const int kq = min((int)sft, A.tb_nk - 1);
      const float tb_t = sft - (float)kq;
      const int tb_off = (A.o_tbtab + ((ti * A.T + tj) * A.tb_nk + kq) * 256 + 4 * g) * 4;      // byte offset inside the weight buffer: 32 bits per lane, the 16 gathers differ in the immediate offset
      const float vm = (valid && xx < 1.f) ? 1.f : 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f32x4 c0 = bload_w(WB, tb_off + (t * 4 + 0) * 64, 0), c1 = bload_w(WB, tb_off + (t * 4 + 1) * 64, 0);
        const f32x4 c2 = bload_w(WB, tb_off + (t * 4 + 2) * 64, 0), c3 = bload_w(WB, tb_off + (t * 4 + 3) * 64, 0);
        x[t] = (c0 + tb_t * (c1 + tb_t * (c2 + tb_t * c3))) * vm;
        bstore(SB, v16, (S::R_DX0 + t) * ROW * 4, (c1 + tb_t * (2.f * c2 + (3.f * tb_t) * c3)) * (vm * tb_invh));
      }
    }
    // ---------------- tensor embedding V^0[lm][u] = w0[l][u] Y[lm] ----------------
    float V[D][UT][4];       // the edge tensor, forward; its gradient, backward: parked in AGPRs (acc_park)
    {
      f32x4 w0[EW];
      lx_lin<AR, 4, EW, false>(WB, wp, x, w0, v16, ring, EpiSave{SB, S::R_W0, v16});
#pragma unroll
      for (int lm = 0; lm < D; ++lm)
#pragma unroll
        for (int t = 0; t < UT; ++t) acc_put4(V[lm][t], lm == 0 ? w0[t] : w0[l_of_lm(lm) * UT + t] * Y[lm]);
    }
    if (ck == 0 && tid == 0) lds.chunk[cpar ^ 1] = claimed;
    __syncthreads();          // aoff visible; previous tile's LDS users done
    PHASEX(PX_EMB);

    // ---------------- layers, forward ----------------
#pragma unroll
    for (int kk = 0; kk < NL; ++kk) {
      const bool last = (kk == NL - 1);
      const int RL = S::R_LAYER(kk, MD);
      float *const envk = lds.env[kk];
      {
        f32x4 om[EW];
        // the backward pass reads the l >= 1 rows only; the last layer's stay in LDS
        if (last) lx_lin<AR, 4, EW, false>(WB, wp, x, om, v16, ring, EpiSaveFromL<UT>{lds.rowsl[uwave], fresh_lane()});
        else lx_lin<AR, 4, EW, false>(WB, wp, x, om, v16, ring, EpiSaveFrom<UT>{{SB, RL + S::O_OM, v16}});
        // environment sum over the centre's edges, one K-tile at a time through the double-buffered stage
#ifndef ABL_NO_ENVSTAGE
#pragma unroll
        for (int t = 0; t < UT; ++t) {
          float *const sp = STQ(t & 1);
#pragma unroll
          for (int lm = 0; lm < D; ++lm) *(f32x4 *)(sp + lm * 16) = lm == 0 ? om[t] : om[l_of_lm(lm) * UT + t] * Y[lm];
          __syncthreads();
          reduce_stage_x<NW>(lds.stage[NSTG == 2 ? (t & 1) : 0], aoffp, envk, na, A.cenv, t, uwave);
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (NSTG == 1) { if (t + 1 < UT) __syncthreads(); }          // one staging buffer: every wave has read K-tile t before t + 1 is written
        }
#endif
        __syncthreads();
      }
      PHASEX(PX_ENV);
      // tensor product, in place per K-tile.  RING_DROP: the weight-fragment ring is NOT carried through the tensor-product phases (no
      // linear runs in them): the fragments prefetched by the previous linear's tail are dropped and requested again under the last
      // half pass, which frees 32 registers where the pressure peaks (one extra L2 round trip per phase, hidden by that half pass)
      f32x4 sc[UT];            // scalar outputs (l3 = 0) of the tensor product: the latent MLP's second input
      {
        const float *en = envk + envoff;
        const float *tp = lds.tp[kk] + 4 * (fresh_lane() >> 4);      // (lane-derived offsets are formed where they are used: as tile-long values they end up in scratch)
#ifndef ABL_NO_FTP
        if (!last) {
#pragma unroll
          for (int t = 0; t < UT; ++t) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              f32x2 vin[D], out[D];
#pragma unroll
              for (int lm = 0; lm < D; ++lm) vin[lm] = acc_get2(V[lm][t], h);
              if (t == UT - 1 && h == 1) lx_prime<AR>(WB, wp, v16, ring);      // see RING_DROP below
              tp_fwd_x<L, false, U>(vin, en + 16 * t + 2 * h, tp + 16 * t + 2 * h, out);
#pragma unroll
              for (int lm = 0; lm < D; ++lm) acc_put2(V[lm][t], h, out[lm]);
              __builtin_amdgcn_sched_barrier(0);
            }
            sc[t] = acc_get4(V[0][t]);
          }
        } else {
#pragma unroll
          for (int t = 0; t < UT; ++t) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              f32x2 vin[D], out[1];
#pragma unroll
              for (int lm = 0; lm < D; ++lm) vin[lm] = acc_get2(V[lm][t], h);
              if (t == UT - 1 && h == 1) lx_prime<AR>(WB, wp, v16, ring);
              tp_fwd_x<L, true, U>(vin, en + 16 * t + 2 * h, tp + 16 * t + 2 * h, out);
              set_half(sc[t], h, out[0]);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
        }
#else
#pragma unroll
        for (int t = 0; t < UT; ++t) sc[t] = acc_get4(V[0][t]) * *(const f32x4 *)(en + 16 * t) * *(const f32x4 *)(tp + 16 * t);
#endif
      }
      PHASEX(PX_TP);
      // latent MLP on [x, scalars]
#ifndef ABL_NO_LAT
      {
        f32x4 cat[4 + UT], z[HT], z2[HT];
#pragma unroll
        for (int t = 0; t < 4; ++t) cat[t] = x[t];
#pragma unroll
        for (int t = 0; t < UT; ++t) cat[4 + t] = sc[t];
        if constexpr (HT == 8) {
          // 128-wide hidden layers: 1 .. MD - 1 save silu' rows to scratch in every model layer; the last saves its raw z rows -- in the last model layer as images 0..7 of the
          // wave's own slots of stage[0].  The chain ping-pongs z / z2 and ends in z2 for MD = 2, in z otherwise.
          if constexpr (MD == 1) {
            if (last) lx_lin<AR, 4 + UT, HT, false>(WB, wp, cat, z, v16, ring, EpiSiluSaveZL{STQ(0), ZIMG});
            else lx_lin<AR, 4 + UT, HT, false>(WB, wp, cat, z, v16, ring, EpiSiluSaveZ{SB, RL + S::O_Z(1), v16});
          } else {
            lx_lin<AR, 4 + UT, HT, false>(WB, wp, cat, z, v16, ring, EpiSiluSaveD{SB, RL + S::O_Z(1), v16});
            if constexpr (MD == 3) lx_lin<AR, HT, HT, false>(WB, wp, z, z2, v16, ring, EpiSiluSaveD{SB, RL + S::O_Z(2), v16});
            f32x4 (&zi)[HT] = MD == 3 ? z2 : z;
            f32x4 (&zo)[HT] = MD == 3 ? z : z2;
            if (last) lx_lin<AR, HT, HT, false>(WB, wp, zi, zo, v16, ring, EpiSiluSaveZL{STQ(0), ZIMG});
            else lx_lin<AR, HT, HT, false>(WB, wp, zi, zo, v16, ring, EpiSiluSaveZ{SB, RL + S::O_Z(MD), v16});
          }
        } else if constexpr (MD == 2) {
          if (last) {          // the last layer's rows: images 0..3 / 4..7 of the wave's own slots of stage[0] (idle until this layer's backward tensor product)
            lx_lin<AR, 4 + UT, 4, false>(WB, wp, cat, z, v16, ring, EpiSiluSaveDL{STQ(0), 0});
            if constexpr (SAVEZ) lx_lin<AR, 4, 4, false>(WB, wp, z, z2, v16, ring, EpiSiluSaveZL{STQ(0), 4});
            else lx_lin<AR, 4, 4, false>(WB, wp, z, z2, v16, ring, EpiSiluSaveDL{STQ(0), 4});
          } else {
            lx_lin<AR, 4 + UT, 4, false>(WB, wp, cat, z, v16, ring, EpiSiluSaveD{SB, RL + S::O_Z(1), v16});
            if constexpr (SAVEZ) lx_lin<AR, 4, 4, false>(WB, wp, z, z2, v16, ring, EpiSiluSaveZ{SB, RL + S::O_Z(2), v16});
            else lx_lin<AR, 4, 4, false>(WB, wp, z, z2, v16, ring, EpiSiluSaveD{SB, RL + S::O_Z(2), v16});
          }
        } else if constexpr (MD == 1) {
          // the only hidden layer is the last one: raw z rows (images 0..3 in the last model layer)
          if (last) lx_lin<AR, 4 + UT, 4, false>(WB, wp, cat, z, v16, ring, EpiSiluSaveZL{STQ(0), ZIMG});
          else lx_lin<AR, 4 + UT, 4, false>(WB, wp, cat, z, v16, ring, EpiSiluSaveZ{SB, RL + S::O_Z(1), v16});
        } else {
          // hidden layer 1: silu' rows to scratch in every model layer (see ZIMG); 2: silu' rows, 3: raw z rows -- in the last model layer images 0..3 / 4..7.
          // The chain ping-pongs z / z2: hidden layer 3's output is back in z.
          lx_lin<AR, 4 + UT, 4, false>(WB, wp, cat, z, v16, ring, EpiSiluSaveD{SB, RL + S::O_Z(1), v16});
          if (last) {
            lx_lin<AR, 4, 4, false>(WB, wp, z, z2, v16, ring, EpiSiluSaveDL{STQ(0), 0});
            lx_lin<AR, 4, 4, false>(WB, wp, z2, z, v16, ring, EpiSiluSaveZL{STQ(0), ZIMG});
          } else {
            lx_lin<AR, 4, 4, false>(WB, wp, z, z2, v16, ring, EpiSiluSaveD{SB, RL + S::O_Z(2), v16});
            lx_lin<AR, 4, 4, false>(WB, wp, z2, z, v16, ring, EpiSiluSaveZ{SB, RL + S::O_Z(3), v16});
          }
        }
        f32x4 (&zl)[HT] = MD == 2 ? z2 : z;             // output of the last hidden layer
        const float ra = lds.res[kk][0], rbf = lds.res[kk][1] * fc;
        f32x4 xn[4];
        if constexpr (SAVEZ) lx_lin<AR, HT, 4, false>(WB, wp, zl, xn, v16, ring, EpiResidualNS<4>{x, ra, rbf});
        else lx_lin<AR, HT, 4, false>(WB, wp, zl, xn, v16, ring, EpiResidual<4>{{SB, RL + S::O_U(MD), v16}, x, ra, rbf});
#pragma unroll
        for (int t = 0; t < 4; ++t) x[t] = xn[t];
      }
#else
      x[0] += sc[0]; x[1] += sc[1]; x[2] += sc[2]; x[3] += sc[3];
#endif
      PHASEX(PX_LAT);
      // channel mixing, in place per (l, m) row -> V^{kk+1}, saved as the next layer's V_in rows
#ifndef ABL_NO_MIX
      if (!last) {
        if (kk + 1 == NL - 1) mix_rows<0, D, UT, true, AR, true>(V, WB, wp, v16, ring, SB, S::R_LAYER(kk + 1, MD) + S::O_VIN(MD), sc, lds.rowsl[uwave], NOML, NVL);
        else mix_rows<0, D, UT, true, AR>(V, WB, wp, v16, ring, SB, S::R_LAYER(kk + 1, MD) + S::O_VIN(MD), sc);
      }
#endif
      PHASEX(PX_MIX);
    }

    // ---------------- read-out ----------------
    // saved rows are requested well ahead of their first use all through the backward pass (their round trip is an L2 miss:
    // 1-2 us, and with one wave per SIMD nothing else covers it): u and silu'(z2) of the last layer under the read-out MFMAs
    f32x4 upre[4], zt[HT], w0pre[L * UT];
    if constexpr (!SAVEZ) load_rows<4>(SB, S::R_LAYER(NL - 1, MD) + S::O_U(MD), upre, v16);
    __builtin_amdgcn_sched_barrier(0);
    f32x4 zr[RT];
    lx_lin<AR, 4, RT, false>(WB, wp, x, zr, v16, ring, EpiNone{});
    f32x4 zr2[RT];           // RD = 2: pre-activations of the read-out's second hidden layer
    if constexpr (RD == 2) {
      f32x4 hr[RT];
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) hr[t][r] = silu1(zr[t][r]);
      lx_lin<AR, RT, RT, false, 0>(WB, wp, hr, zr2, v16, ring, EpiNone{});
    }
    f32x4 (&zo)[RT] = RD == 2 ? zr2 : zr;       // pre-activations of the last hidden layer
    f32x4 wo1[RT];           // the read-out's final R -> 1 vector (out.w1, or out.w2 of a depth-2 read-out), R = 16 RT
#pragma unroll
    for (int t = 0; t < RT; ++t) wo1[t] = *(const f32x4 *)(Wb + A.o_out1 + 16 * t + 4 * g);
    float eps = 0.f;
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) eps += silu1(zo[t][r]) * wo1[t][r];
    eps = gsum(eps);
    pin(eps);

    // =========================== backward ===========================
    // f16x2: the backward pass runs scaled by a power of two (fused_h.h) -- per CENTRE TYPE since round 6: the exponent of this centre type's own upstream
    // gradient (every edge of a centre shares it); its inverse waits in the slot's pad floats of the staging tile (never staged, never reduced)
    float bsc = 1.f;
    if constexpr (AR == 3) {
      int bex;
      (void)frexpf(lds.scale[ti] * A.cenv, &bex);
      bex = min(max(bex, -100), 100);         // a subnormal or huge scale (bex ~ -130 for 1e-39) would make one of 2^-bex, 2^bex inf: both stay finite and normal
      bsc = ldexpf(1.f, -bex);
      if (g == 0) lds.stage[0][s * STG_LD + D * 16] = ldexpf(1.f, bex);
    }
    const float deps = valid ? lds.scale[ti] * A.cenv * bsc : 0.f;
    f32x4 dx[4];
    {
      f32x4 dzr[RT];
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) dzr[t][r] = deps * wo1[t][r] * dsilu1(zo[t][r]);
      if constexpr (RD == 2) {
        // dzr holds the gradient of zr2: back through out.w1^T and the first hidden layer's SiLU (linear in deps, so the f16x2 power-of-two scale passes through)
        f32x4 dhr[RT];
        lx_lin<AR, RT, RT, false, 4>(WB, wp, dzr, dhr, v16, ring, EpiNone{});
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) dzr[t][r] = dhr[t][r] * dsilu1(zr[t][r]);
      }
      lx_lin<AR, RT, 4, false>(WB, wp, dzr, dx, v16, ring, EpiNone{});
    }
#pragma unroll
    for (int t = 0; t < HT; ++t) zt[t] = stg_load(STQ(0), ZIMG + t);        // the last layer's last hidden layer rows, from the staging tile
    float dfc_part = 0.f;
    float dY[D];
#pragma unroll
    for (int lm = 0; lm < D; ++lm) dY[lm] = 0.f;
    PHASEX(PX_OUT);

#pragma unroll
    for (int kk = NL - 1; kk >= 0; --kk) {
      const bool last = (kk == NL - 1);
      const int RL = S::R_LAYER(kk, MD);
      f32x4 ds[UT];
      {
        f32x4 du[HT], dh[HT];
        f32x4 rows1[HT];         // silu' of the hidden layer below the last (MD >= 2): first used one linear from here
        if constexpr (MD >= 2) {
          if (HT == 4 && last) {   // (HT = 8: in scratch in every model layer)
#pragma unroll
            for (int t = 0; t < 4; ++t) rows1[t] = stg_load(STQ(0), t);
          } else load_rows<HT>(SB, RL + S::O_Z(MD - 1), rows1, v16);
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (SAVEZ) {
          // the u rows are not saved (fused.hip: SAVEZ): <u, g> falls out of the epilogue of the first backward linear, fed with the unscaled gradient
          const float ra = lds.res[kk][0], rb = lds.res[kk][1];
          float ug = 0.f;
          lx_lin<AR, 4, HT, false>(WB, wp, dx, dh, v16, ring, EpiMulSiluZ<HT>{zt, rb * fc, ug});
#pragma unroll
          for (int t = 0; t < 4; ++t) dx[t] = ra * dx[t];
          dfc_part += rb * ug;
          pin(dfc_part);
        } else {
          const float ra = lds.res[kk][0], rb = lds.res[kk][1];
          f32x4 accv = upre[0] * dx[0];
#pragma unroll
          for (int t = 1; t < 4; ++t) accv += upre[t] * dx[t];
          const float rbfc = rb * fc;
#pragma unroll
          for (int t = 0; t < 4; ++t) { du[t] = rbfc * dx[t]; dx[t] = ra * dx[t]; }
          dfc_part += rb * hsum4(accv);
          pin(dfc_part);
          lx_lin<AR, 4, 4, false>(WB, wp, du, dh, v16, ring, EpiMulRows<4>{zt});
        }
        // down the hidden layers: g_{h-1} = (g_h W_h^T) * silu'(z_{h-1}), then dcat = g_1 W_0^T
        f32x4 dcat[4 + UT];
        if constexpr (MD == 2) {
          lx_lin<AR, HT, HT, false>(WB, wp, dh, du, v16, ring, EpiMulRows<HT>{rows1});
          lx_lin<AR, HT, 4 + UT, false>(WB, wp, du, dcat, v16, ring, EpiNone{});
        } else if constexpr (MD == 1) {
          lx_lin<AR, HT, 4 + UT, false>(WB, wp, dh, dcat, v16, ring, EpiNone{});
        } else {
          // silu' of hidden layer 1 (scratch in every model layer): requested one linear ahead, after the stage reads of rows1 above
          f32x4 rows0[HT];
          load_rows<HT>(SB, RL + S::O_Z(1), rows0, v16);
          __builtin_amdgcn_sched_barrier(0);
          lx_lin<AR, HT, HT, false>(WB, wp, dh, du, v16, ring, EpiMulRows<HT>{rows1});
          lx_lin<AR, HT, HT, false>(WB, wp, du, dh, v16, ring, EpiMulRows<HT>{rows0});
          lx_lin<AR, HT, 4 + UT, false>(WB, wp, dh, dcat, v16, ring, EpiNone{});
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) dx[t] += dcat[t];
#pragma unroll
        for (int t = 0; t < UT; ++t) ds[t] = dcat[4 + t];
      }
      PHASEX(PX_BLAT);
      // mix^T in place per (l, m) row: V holds dE/dV^{kk+1}, becomes dE/dV' (tensor-product output gradient)
      if (!last) mix_rows<0, D, UT, false, AR>(V, WB, wp, v16, ring, SB, 0, ds);
      PHASEX(PX_BMIX);
      // tensor-product gradient in place per K-tile; the per-edge environment gradient goes through the stage
      {
        const float *en = lds.env[kk] + envoff;
        const float *tp = lds.tp[kk] + 4 * (fresh_lane() >> 4);      // (lane-derived offsets are formed where they are used: as tile-long values they end up in scratch)
        // the saved input rows V^{kk}[.][t] (w0 rows for the first layer) of half pass (t, h) are requested one half pass
        // ahead: their round trip (L2 miss: 1-2 us) runs under the previous half pass
        // saved input rows of half pass i = 2 t + h live in vpre2[i & 1] and are requested TWO half passes ahead (an HBM round trip
        // under load is ~2 us, one half pass ~1 us)
        f32x2 vpre2[2][D];
        f32x4 omall[L * UT];      // omega rows of l >= 1 (all K-tiles) for the step after this one: requested before the last reduction
        auto request_vin = [&](int i) {
          const int t = i >> 1, h = i & 1;
          if (kk > 0) {
#pragma unroll
            for (int lm = 0; lm < D; ++lm) {
              if (last && lm * UT + t < NVL) vpre2[i & 1][lm] = *(const f32x2 *)(lds.rowsl[uwave] + (NOML + lm * UT + t) * ROW + fresh_lane() * 4 + 2 * h);
              else vpre2[i & 1][lm] = bload_half(SB, v16 + 8 * h, (RL + S::O_VIN(MD) + lm * UT + t) * ROW * 4);
            }
          } else {
#pragma unroll
            for (int l = 0; l <= L; ++l) vpre2[i & 1][l] = bload_half(SB, v16 + 8 * h, (S::R_W0 + l * UT + t) * ROW * 4);
          }
        };
        request_vin(0);
        request_vin(1);
#pragma unroll
        for (int t = 0; t < UT; ++t) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            f32x2 vin[D], a[D], b[D], ee[D];
#pragma unroll
            for (int lm = 0; lm < D; ++lm) vin[lm] = vpre2[h][lm];
#pragma unroll
            for (int lm = 0; lm < D; ++lm) ee[lm] = *(const f32x2 *)(en + 16 * t + 2 * h + lm * U);
            f32x2 pwh[NP];          // path weights of this half pass: one batch of LDS reads, one wait
#pragma unroll
            for (int pth = 0; pth < NP; ++pth) pwh[pth] = *(const f32x2 *)(tp + 16 * t + 2 * h + pth * U);
            __builtin_amdgcn_sched_barrier(0);
            // next half pass's rows: requested AFTER this half pass's LDS reads -- a spilled LDS address reloaded between the
            // request and those reads would wait on vmcnt(0), i.e. on the rows just requested (loads return in order)
            // the stage pointer is needed after the tensor-product arithmetic: if it sits in a scratch slot, reload it NOW -- after
            // the request below a reload waits (vmcnt(0), in-order return) for the rows coming from HBM
            float *const sp = STQ(t & 1);
            if (2 * t + h + 2 < 2 * UT) request_vin(2 * t + h + 2);
            __builtin_amdgcn_sched_barrier(0);
            if (!last) {
              f32x2 gg[D];
#pragma unroll
              for (int lm = 0; lm < D; ++lm) gg[lm] = acc_get2(V[lm][t], h);
              tp_bwd_half<L, false, U, 0>(ee, pwh, gg, a);
              __builtin_amdgcn_sched_barrier(0);
              if (kk == 0) {
#pragma unroll
                for (int lm = D - 1; lm >= 1; --lm) vin[lm] = vin[l_of_lm(lm)] * Y[lm];
              }
              tp_bwd_half<L, false, U, 1>(vin, pwh, gg, b);
            } else {
              f32x2 gg[1];
              gg[0] = half_of(ds[t], h);
              tp_bwd_half<L, true, U, 0>(ee, pwh, gg, a);
              __builtin_amdgcn_sched_barrier(0);
              if (kk == 0) {
#pragma unroll
                for (int lm = D - 1; lm >= 1; --lm) vin[lm] = vin[l_of_lm(lm)] * Y[lm];
              }
              tp_bwd_half<L, true, U, 1>(vin, pwh, gg, b);
            }
#pragma unroll
            for (int lm = 0; lm < D; ++lm) { acc_put2(V[lm][t], h, a[lm]); *(f32x2 *)(sp + lm * 16 + 2 * h) = b[lm]; }
            __builtin_amdgcn_sched_barrier(0);
          }
          if (t == UT - 1) {
            if (last) {
#pragma unroll
              for (int r = 0; r < L * UT; ++r) omall[r] = lrow_load(lds.rowsl[uwave], r, fresh_lane());
            } else load_rows<L * UT>(SB, RL + S::O_OM + UT, omall, v16);
          }
          __syncthreads();
          reduce_stage_x<NW>(lds.stage[NSTG == 2 ? (t & 1) : 0], aoffp, lds.denv, na, A.cenv, t, uwave);
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (NSTG == 1) { if (t + 1 < UT) __syncthreads(); }
        }
        __syncthreads();
      PHASEX(PX_BTP);
      // environment weights backward: d omega[l][u] = sum_m denv[lm][u] Y[lm];  dY[lm] += sum_u denv[lm][u] omega[l][u]
        f32x4 dom[EW];
        const float *dn = lds.denv + envoff;
#pragma unroll
        for (int t = 0; t < UT; ++t) {
          f32x4 omr[L + 1];
#pragma unroll
          for (int l = 1; l <= L; ++l) omr[l] = omall[(l - 1) * UT + t];
#pragma unroll
          for (int l = 0; l <= L; ++l) dom[l * UT + t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int lm = 0; lm < D; ++lm) {
            const f32x4 dv = *(const f32x4 *)(dn + lm * U + 16 * t);
            if (lm == 0) dom[t] = dv;
            else {
              dom[l_of_lm(lm) * UT + t] += dv * Y[lm];
              dY[lm] += hsum4(dv * omr[l_of_lm(lm)]);
            }
          }
#pragma unroll
          for (int lm = 1; lm < D; ++lm) pin(dY[lm]);        // see pin(): keeps the sums where they are computed
          __builtin_amdgcn_sched_barrier(0);
        }
        lx_prime<AR>(WB, wp, v16, ring);          // RING_DROP: requested again only now -- the d omega / dY arithmetic above needs the registers
        // next iteration's u / silu'(z2) rows (or the l >= 1 embedding weights for the last step) under this linear
        if (kk > 0) {
          if constexpr (!SAVEZ) load_rows<4>(SB, S::R_LAYER(kk - 1, MD) + S::O_U(MD), upre, v16);
          load_rows<HT>(SB, S::R_LAYER(kk - 1, MD) + S::O_Z(MD), zt, v16);
        } else load_rows<L * UT>(SB, S::R_W0 + UT, w0pre, v16);
        __builtin_amdgcn_sched_barrier(0);
        lx_lin<AR, EW, 4, true>(WB, wp, dom, dx, v16, ring, EpiNone{});
      }
      PHASEX(PX_BENV);
    }
    // ---------------- embedding backward: V holds dE/dV^0 ----------------
    {
      f32x4 dw0[EW];
#pragma unroll
      for (int t = 0; t < UT; ++t) {
        f32x4 w0r[L + 1];
#pragma unroll
        for (int l = 1; l <= L; ++l) w0r[l] = w0pre[(l - 1) * UT + t];
#pragma unroll
        for (int l = 0; l <= L; ++l) dw0[l * UT + t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int lm = 0; lm < D; ++lm) {
          const f32x4 dv = acc_get4(V[lm][t]);
          if (lm == 0) dw0[t] = dv;
          else {
            dw0[l_of_lm(lm) * UT + t] += dv * Y[lm];
            dY[lm] += hsum4(dv * w0r[l_of_lm(lm)]);
          }
        }
#pragma unroll
        for (int lm = 1; lm < D; ++lm) pin(dY[lm]);
        __builtin_amdgcn_sched_barrier(0);
      }
      lx_lin<AR, EW, 4, true>(WB, wp, dw0, dx, v16, ring, EpiNone{});
      wp = A.o_stream;                                                     // last linear of the tile (wrap-around copy follows it)
    }
    PHASEX(PX_BEMB);
    // ---------------- two-body embedding backward ----------------
    float dd_part;
    {
      f32x4 rows[4];
      load_rows<4>(SB, S::R_DX0, rows, v16);
      f32x4 accv = dx[0] * rows[0];
#pragma unroll
      for (int t = 1; t < 4; ++t) accv += dx[t] * rows[t];
      dd_part = hsum4(accv);
      pin(dd_part);
    }
    // ---------------- geometry backward, outputs ----------------
    {
      const float ibs = AR == 3 ? lds.stage[0][s * STG_LD + D * 16] : 1.f;      // this slot's inverse backward scale (per centre type, written at the start of the backward pass)
      const float dfc_tot = gsum(dfc_part) * ibs;
      const float dd = dfc_tot * (dfc_dx / rc) + gsum(dd_part) * ibs;
      float yv[D];
#pragma unroll
      for (int lm = 1; lm < D; ++lm) yv[lm] = gsum(dY[lm]) * ibs;
      // G = sum_lm dE/dY_lm * dY_lm/dn (n treated as a free vector), then projected onto the sphere
      float Gx = C3 * yv[3], Gy = C3 * yv[1], Gz = C3 * yv[2];
      if constexpr (L >= 2) {
        Gx += C15 * (yv[4] * ny + yv[7] * nz + yv[8] * nx) - 2.f * C5H * yv[6] * nx;
        Gy += C15 * (yv[4] * nx + yv[5] * nz - yv[8] * ny) - 2.f * C5H * yv[6] * ny;
        Gz += C15 * (yv[5] * ny + yv[7] * nx) + 4.f * C5H * yv[6] * nz;
      }
      const float gn = Gx * nx + Gy * ny + Gz * nz;
      const float gx = dd * nx + (Gx - gn * nx) * inv;
      const float gy = dd * ny + (Gy - gn * ny) * inv;
      const float gz = dd * nz + (Gz - gn * nz) * inv;
      const float m = valid ? 1.f : 0.f;
      if (AR == 3 && valid && !(fabsf(gx) + fabsf(gy) + fabsf(gz) + fabsf(eps) < 3.0e38f)) *A.err = 1;      // inf / NaN: an operand left float16's range
      float *const st = lds.stage[0] + s * STG_LD;
      if (g == 0) {
        st[0] = m * gx; st[1] = m * gy; st[2] = m * gz; st[3] = m * eps;
        if (valid) {
          atomicAdd(&A.f[3 * (size_t)jat], -(double)gx);
          atomicAdd(&A.f[3 * (size_t)jat + 1], -(double)gy);
          atomicAdd(&A.f[3 * (size_t)jat + 2], -(double)gz);
        }
      }
      if constexpr (VA) vatom_scatter(A.vatom, jat, g, valid, rx, ry, rz, gx, gy, gz);
      float w6[6] = {-m * rx * gx, -m * ry * gy, -m * rz * gz, -m * 0.5f * (rx * gy + ry * gx),
                     -m * 0.5f * (rx * gz + rz * gx), -m * 0.5f * (ry * gz + rz * gy)};
#pragma unroll
      for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) w6[c] += __shfl_xor(w6[c], off, 64);
      }
      if (lane < 6) {
        const float mine = lane == 0 ? w6[0] : lane == 1 ? w6[1] : lane == 2 ? w6[2] : lane == 3 ? w6[3] : lane == 4 ? w6[4] : w6[5];
        lds.virw[wave][lane] += (double)mine;
      }
    }
    __syncthreads();
    {
      const int col = tid & 3, part = (tid >> 2) & 3;
      float sum = 0.f;
      if (ca < na)
        for (int sl = aoffp[ca] + part; sl < aoffp[ca + 1]; sl += 4) sum += lds.stage[0][sl * STG_LD + col];
      sum += __shfl_xor(sum, 4, 64);
      sum += __shfl_xor(sum, 8, 64);
      if (ca < na && part == 0) {
        if (col < 3) atomicAdd(&A.f[3 * (size_t)c_i + col], (double)sum);
        else {
          const float ei = lds.scale[c_t] * (sum * A.cenv) + lds.shift[c_t];
          if (A.eatom) A.eatom[c_i] = (double)ei;
          lds.eacc[ca] += (double)ei;
        }
      }
    }
    // no trailing barrier: the next tile's first staging write sits behind the barrier after its embedding linear
    PHASEX(PX_FIN);
    if (++ck == A.tchunk) { ck = 0; cpar ^= 1; cbase = __builtin_amdgcn_readfirstlane(lds.chunk[cpar]); }
  }
  __syncthreads();
  if (tid == 0) {
    for (int a = 0; a < MAXA; ++a) acc_part += lds.eacc[a];
  } else if (tid >= 64 && tid < 70) {
    for (int w = 0; w < NW; ++w) acc_part += lds.virw[w][tid - 64];
  }
  if (PROF && lane == 0) {
#pragma unroll
    for (int k = 0; k < PX_N; ++k) atomicAdd((unsigned long long *)&A.prof[k], (unsigned long long)pacc[k]);
  }
  if (tid == 0) A.partial[7 * (size_t)blockIdx.x] = acc_part;
  if (tid >= 64 && tid < 70) A.partial[7 * (size_t)blockIdx.x + 1 + (tid - 64)] = acc_part;
}

// ---------------------------------------------------------------------------- host side
// This file is compiled in parts (Makefile): AHIP_LX_PART 0 = the host side and the instances of part 0, n = the instances of part n alone (2: with AHIP_NO_ACC_PARK);
// which instances a part holds is fused_shapes.h: FUSED_INSTANCES
#ifndef AHIP_LX_PART
#define AHIP_LX_PART 0
#endif
// (the static_asserts: what a dispatch list names is in that table -- {family, arithmetic, -, MD, RD, WF, RF, option, NW, NL, variant} -- and in this part)
void fusedlx_launch_rd2(int nl, int var, int md, int grid, hipStream_t s, const FusedLxArgs &A);
void fusedlx_launch_w8(int nl, int ar, int var, int grid, hipStream_t s, const FusedLxArgs &A);
void fusedlx_launch_m(int nl, int var, int md, int grid, hipStream_t s, const FusedLxArgs &A);
void fusedlx_launch_q(int nl, int var, int md, int grid, hipStream_t s, const FusedLxArgs &A);
#if AHIP_LX_PART == 4
void fusedlx_launch_q(int nl, int var, int md, int grid, hipStream_t s, const FusedLxArgs &A) {      // fused_lx_q.o: RT = 4
  dispatch<Choices<1, 2, 3>, Choices<VAR_VA, VAR_PLAIN>, Choices<1, 3, 2>>([&](auto nl, auto v, auto md) {
    static_assert(fused_part_holds(AHIP_LX_PART, {FusedFamily::lx32, 3, true, md, 1, 64, 64, false, 4, nl, v}), "not in FUSED_INSTANCES");
    hipLaunchKernelGGL((k_fused_lx<4, nl, false, 3, v == VAR_VA, md, 1, 4, 4>), dim3(grid), dim3(4 * 64), 0, s, A);
  }, nl, var, md);
}
#elif AHIP_LX_PART == 3
void fusedlx_launch_m(int nl, int var, int md, int grid, hipStream_t s, const FusedLxArgs &A) {      // fused_lx_m.o: HT = 8
  dispatch<Choices<1, 2, 3>, Choices<VAR_VA, VAR_PLAIN>, Choices<1, 3, 2>>([&](auto nl, auto v, auto md) {
    static_assert(fused_part_holds(AHIP_LX_PART, {FusedFamily::lx32, 3, true, md, 1, 128, 32, false, 4, nl, v}), "not in FUSED_INSTANCES");
    hipLaunchKernelGGL((k_fused_lx<4, nl, false, 3, v == VAR_VA, md, 1, 8>), dim3(grid), dim3(4 * 64), 0, s, A);
  }, nl, var, md);
}
#elif AHIP_LX_PART == 1
void fusedlx_launch_rd2(int nl, int var, int md, int grid, hipStream_t s, const FusedLxArgs &A) {      // fused_lx_r.o: RD = 2
  dispatch<Choices<1, 2, 3>, Choices<VAR_VA, VAR_PLAIN>, Choices<1, 3, 2>>([&](auto nl, auto v, auto md) {
    static_assert(fused_part_holds(AHIP_LX_PART, {FusedFamily::lx32, 3, true, md, 2, 64, 32, false, 4, nl, v}), "not in FUSED_INSTANCES");
    hipLaunchKernelGGL((k_fused_lx<4, nl, false, 3, v == VAR_VA, md, 2>), dim3(grid), dim3(4 * 64), 0, s, A);
  }, nl, var, md);
}
#elif AHIP_LX_PART == 2
#ifndef AHIP_NO_ACC_PARK
#error "the 8-wave instances have 256 registers per wave: no AGPR park (build fused_lx_w.o with -DAHIP_NO_ACC_PARK)"
#endif
void fusedlx_launch_w8(int nl, int ar, int var, int grid, hipStream_t s, const FusedLxArgs &A) {      // fused_lx_w.o: NW = 8
  dispatch<Choices<1, 2, 3>, Choices<3, 0>, Choices<VAR_VA, VAR_PLAIN>>([&](auto nl, auto ar, auto v) {
    static_assert(fused_part_holds(AHIP_LX_PART, {FusedFamily::lx32, ar, true, 2, 1, 64, 32, false, 8, nl, v}), "not in FUSED_INSTANCES");
    hipLaunchKernelGGL((k_fused_lx<8, nl, false, ar, v == VAR_VA>), dim3(grid), dim3(8 * 64), 0, s, A);
  }, nl, ar, var);
}
#else

// the gate itself: fused_shapes.h
bool fusedlx_model_supported(const Model &m, std::string *why) { return fused_wide_supported(m.hm, resolve_arith(m, true), why, fused_n_active(m), fused_lx64_w128(m)); }
static_assert(LX_MAXNL == 3, "fused_shapes.h: 1..3 layers");

// k_fused_lx's weight stream, in the order one tile consumes it: whole-matrix fragments (see k_fused_lx)
static int lx_stream(std::vector<float> &w, FusedLxArgs &A, const HostModel &h, Arith arith) {
  using S = ShapeX<4>;          // (the stream does not depend on the tile shape)
  constexpr int L = S::L, U = S::U, D = S::D;
  const int NL = h.num_layers, MD = h.mlp_depth;      // latent MLP: lat.w0 ([x, scalars] -> W), lat.w1 .. lat.w{MD-1} (W -> W), output linear lat.w{MD} (W -> 64)
  const int W = h.mlp_width;                          // hidden width at the kernel's shape: 64 or 128 (fused_shapes.h: FUSED_WF, FUSED_WF2)
  const int RF = h.readout_width;                     // read-out width at the kernel's shape: 32 or 64 (FUSED_RF, FUSED_RF2)
  auto T_ = [&](const std::string &name) -> const double * { return h.get(name).data.data(); };
  int h_flags = 0;        // float16 range findings over the weight stream (engine.h: H_RANGE_*)
  auto frag = [&](const double *W, int K, int N, int ldw) {
    if (arith == AR_F16X2) h_flags |= append_frag_h(w, W, K, N, ldw);
    else append_frag(w, W, K, N, ldw);
  };
  auto fwd = [&](const double *W, int K, int N) { frag(W, K, N, N); };
  auto bwd = [&](const double *W, int K, int N) { auto t = transpose(W, K, N); frag(t.data(), N, K, K); };
  // one channel-mixing row; the last (ninth) row is padded to 64 output columns (8 fragments, see mix_rows)
  static_assert(S::UT == 2 && D % 2 == 1, "rows alternate the ring phase");
  auto mixfrag = [&](const double *Wl, int lm, bool transposed) {
    std::vector<double> m2((size_t)U * U);
    for (int a = 0; a < U; ++a)
      for (int b = 0; b < U; ++b) m2[(size_t)a * U + b] = transposed ? Wl[(size_t)b * U + a] : Wl[(size_t)a * U + b];
    if (lm == D - 1) {
      std::vector<double> pad((size_t)U * 2 * U, 0.0);
      for (int a = 0; a < U; ++a)
        for (int b = 0; b < U; ++b) pad[(size_t)a * 2 * U + b] = m2[(size_t)a * U + b];
      frag(pad.data(), U, 2 * U, 2 * U);
    } else frag(m2.data(), U, U, U);
  };
  A.o_stream = w_mark(w);
  const size_t stream0 = w.size();
  fwd(T_("emb.w"), 64, U * (L + 1));
  for (int k = 0; k < NL; ++k) {
    const std::string lk = "l" + std::to_string(k + 1);
    fwd(T_(lk + ".env"), 64, U * (L + 1));
    fwd(T_(lk + ".lat.w0"), 64 + U, W);
    for (int hl = 1; hl <= MD; ++hl) fwd(T_(lk + ".lat.w" + std::to_string(hl)), W, hl < MD ? W : 64);
    if (k < NL - 1) {
      const double *mx = T_(lk + ".mix");            // [L+1][U][U]; block l serves its 2l+1 components
      for (int lm = 0; lm < D; ++lm) mixfrag(mx + (size_t)l_of_lm(lm) * U * U, lm, false);
    }
  }
  fwd(T_("out.w0"), 64, RF);
  if (h.readout_depth == 2) {      // the read-out's second hidden layer, forward and transposed: half a ring each (k_fused_lx: RD; RF = 32 there)
    fwd(T_("out.w1"), RF, RF);
    bwd(T_("out.w1"), RF, RF);
  }
  bwd(T_("out.w0"), 64, RF);
  for (int k = NL - 1; k >= 0; --k) {
    const std::string lk = "l" + std::to_string(k + 1);
    for (int hl = MD; hl >= 1; --hl) bwd(T_(lk + ".lat.w" + std::to_string(hl)), W, hl < MD ? W : 64);
    bwd(T_(lk + ".lat.w0"), 64 + U, W);
    if (k < NL - 1) {
      const double *mx = T_(lk + ".mix");
      for (int lm = 0; lm < D; ++lm) mixfrag(mx + (size_t)l_of_lm(lm) * U * U, lm, true);
    }
    bwd(T_(lk + ".env"), 64, U * (L + 1));
  }
  bwd(T_("emb.w"), 64, U * (L + 1));
  for (size_t i = 0; i < (size_t)RING * 256; ++i) w.push_back(w[stream0 + i]);      // wrap-around copy
  return h_flags;
}

bool fusedlx_run(Model &m, const ComputeArgs &a, std::string *why) {
  const int max_slots = lx_max_tile_slots(m, FusedFamily::lx32);
  if (!lx_list_fits(m, why, max_slots)) return false;
  const bool w128 = fused_WF(m.hm) == FUSED_WF2;       // MLP width 65..128: the HT = 8 instances, whose row map sizes the per-wave scratch
  FusedLxState &st = w128 ? lx_prepare<ShapeX<4, 8>>(m, m.fusedlx_state, nullptr, false, lx_stream, 4)
                          : lx_prepare<ShapeX<4>>(m, m.fusedlx_state, nullptr, false, lx_stream, max_slots > LX_TILE_SLOTS ? 8 : 4);
  static_assert(PX_N == LX_NPHASE, "profile phases");
  const FusedInstanceKey key{FusedFamily::lx32, st.arith, true, st.md, st.rd, 16 * st.ht, 16 * st.rt};
  // Tile shape (4 waves / 64 slots or 8 waves / 128 slots, option wide_tile=auto) from the largest degree of THIS list, as k_fused does (fused.hip: fused_run): on the
  // host where it is known or bounded by the list's rows, else both shapes are launched and the device word decides (nw = 0)
  int nw = 4;
  if (max_slots > LX_TILE_SLOTS) {
    if (!m.counts_pending) nw = m.last_max_deg <= LX_TILE_SLOTS ? 4 : 8;
    else nw = (m.max_list_row >= 0 && m.max_list_row <= LX_TILE_SLOTS) ? 4 : 0;
  }
  lx_run<ShapeX<4>, ShapeX<8>>(m, a, st, "fused_lx", key, [&](const FusedLxArgs &A, int grid, int var, int part) {
    switch (part) {
      case 2: fusedlx_launch_w8(A.NL, st.arith, var, grid, a.stream, A); break;
      case 3: fusedlx_launch_m(A.NL, var, st.md, grid, a.stream, A); break;
      case 4: fusedlx_launch_q(A.NL, var, st.md, grid, a.stream, A); break;
      case 1: fusedlx_launch_rd2(A.NL, var, st.md, grid, a.stream, A); break;
      case 0:
        dispatch<Choices<1, 2, 3>, Choices<3, 0>, Variants, Choices<1, 3, 2>>([&](auto nl, auto ar, auto v, auto md) {
          if constexpr (fused_part_holds(AHIP_LX_PART, {FusedFamily::lx32, ar, true, md, 1, 64, 32, false, 4, nl, v}))         // (the gate and lx_run never send anything else)
            hipLaunchKernelGGL((k_fused_lx<4, nl, v == VAR_PROF, ar, v == VAR_VA, md>), dim3(grid), dim3(4 * 64), 0, a.stream, A);
          else throw StateError("k_fused_lx: not an instance of part 0");
        }, A.NL, st.arith, var, st.md);
        break;
      default: throw StateError("k_fused_lx: no launch function for part " + std::to_string(part));
    }
  }, nw);
  return true;
}

void fusedlx_free(Model &m) {
  lx_free(m.fusedlx_state);
  lx_free(m.fusedlx2_state);
}

#endif   // AHIP_LX_PART
}  // namespace ahip

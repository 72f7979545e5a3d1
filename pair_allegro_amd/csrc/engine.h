// Internal engine state shared by the C-ABI (allegro_hip.hip), the generic path
// (generic_engine.h) and the fused MFMA path (fused.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <map>
#include <stdexcept>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "arith_policy.h"
#include "cell_geom.h"
#include "fused_shapes.h"
#include "model_io.h"
#include "prims.h"

namespace ahip {

// (HipError, ArgError, StateError, UnsupportedError: fused_shapes.h)
#define AHIP_CHECK(expr)                                                                       \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess)                                                                      \
      throw ahip::HipError(std::string(#expr) + " failed: " + hipGetErrorString(_e) + " (" +   \
                           __FILE__ + ":" + std::to_string(__LINE__) + ")");                   \
  } while (0)

// grow-only device buffer
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  template <typename T> T *as() const { return (T *)p; }
  void reserve(size_t bytes) {
    if (bytes <= cap) return;
    if (p) AHIP_CHECK(hipFree(p));
    p = nullptr; cap = 0;
    size_t want = bytes + bytes / 16 + 256;          // 6 % head-room: shape hysteresis like the
    AHIP_CHECK(hipMalloc(&p, want));                   // Kokkos path (pair_nequip_allegro_kokkos.cpp:218-229)
    cap = want;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// bump allocator over one DevBuf; first pass measures, second pass hands out pointers
struct Arena {
  char *base = nullptr;
  size_t off = 0;
  bool measuring = true;
  template <typename T> T *get(size_t n) {
    size_t bytes = (n * sizeof(T) + 255) & ~size_t(255);
    T *r = measuring ? nullptr : (T *)(base + off);
    off += bytes;
    return r;
  }
};

template <typename T> struct DeviceWeights {
  std::map<std::string, T *> w;
  std::vector<void *> owned;
  bool ready = false;
  T *get(const std::string &n) const {
    auto it = w.find(n);
    if (it == w.end()) throw StateError("device weight '" + n + "' missing");
    return it->second;
  }
};

extern std::atomic<int> g_models_alive;     // models of this process (allegro_hip.hip)

// Stage timing (option timing=1): HIP events on the launch stream around every stage of a call.  Nothing waits for them when they are recorded
// (round 4: reading them back at the end of every call was a full synchronisation per ahip_compute_dev*); the pairs queue up in a ring and are
// turned into milliseconds when the caller asks (ahip_get_timings: the sum and the number of launches per stage since the last call of it).
struct TimingSlot {
  std::string name;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ring;      // event pairs, reused round-robin
  size_t head = 0, tail = 0;                                // pairs [tail, head) are recorded and not yet read
  double sum_ms = 0; long long count = 0;                   // read so far, not yet reported
};
static constexpr size_t TIMING_RING = 1024;

struct FusedState;       // fused.hip
struct FusedLxState;     // fused_lx_common.h

struct Model {
  HostModel hm;
  int device = 0;
  bool counted = false;                     // included in g_models_alive
  int D = 1, Ka = 0;
  std::vector<double> rcut_model_host;      // [T*T]

  // options
  // options (each enum with its words, in the order of the enumerators: arith_policy.h, word_index)
  enum class Path { Auto, Fused, Generic };
  static constexpr const char *PATH_WORDS = "auto|fused|generic";
  enum class Precision { Model, Float64 };
  static constexpr const char *PRECISION_WORDS = "model|float64";
  enum class TilePack { Auto, Separate, Fused };
  static constexpr const char *TILE_PACK_WORDS = "auto|separate|fused";
  enum class EdgeSchedule { Auto, Static, Dynamic };
  static constexpr const char *EDGE_SCHEDULE_WORDS = "auto|static|dynamic";
  enum class DenseCentres { Whole, Split };
  static constexpr const char *DENSE_CENTRES_WORDS = "whole|split";
  enum class WideTile { S64, Auto };
  static constexpr const char *WIDE_TILE_WORDS = "64|auto";
  enum class Lx64MlpWidth { W64, Auto };
  static constexpr const char *LX64_MLP_WIDTH_WORDS = "64|auto";
  enum class EnvBackward { Auto, Centre, Edge };
  static constexpr const char *ENV_BACKWARD_WORDS = "auto|centre|edge";
  Path opt_path = Path::Auto;
  Precision opt_precision = Precision::Model;
  FusedTb opt_fused_tb = FusedTb::Table;    // table | mlp: two-body embedding of the fused kernel from the spline table or as an MLP
  ArithState arith;                         // option fused_arith (auto | f32 | f16x2 | bf16x3 | tf32eq) and what auto has decided so far: arith_policy.h
  DevBuf b_chk;                             // self-check: two force arrays + the 2-word reduction
  // A model narrower than a fused kernel's fixed widths runs on it zero-padded (round 6; model_io.h: pad_host_model): S <= 64 scalars, MLP width <= 64 (65..128: padded
  // to the second hidden width 128 of k_fused / k_fused_lx, fused_shapes.h: fused_WF), read-out width <= 32 (33..64: padded to the second read-out width 64, fused_RF), U <= 32 tensor features on k_fused / k_fused_lx, <= 64 on k_fused_lx2 (an l_max = 1 model with 33..64 features lifted to l_max = 2 as well:
  // fused_shapes.h).  hm stays the model as loaded (layer-at-a-time kernels, metadata).
  HostModel hm_fused;
  bool hm_fused_ready = false;
  // Active types (fused_shapes.h): the model types the caller's type mapping can produce.  While `active` is non-empty the fused side runs on the model restricted to
  // it (fused_host_model: subset_host_model, then padded / lifted) with compact type slots 0 .. A - 1 in ascending model-type order; the three writers of fused-side
  // types (edges.hip: k_pack_xt; fused_common.h: k_centre_info / k_pack_small, k_edge_types) translate through the byte table slot_dev.  Everything else -- hm, the
  // layer-at-a-time kernels, heavy centres, ghost rows of atomic_energy, ahip_model_meta -- keeps full model types and full tables.
  std::vector<int> active;                   // the subset in force (strictly ascending); empty: none, the fused side sees every type of the model
  std::vector<int> active_set;               // set by ahip_set_active_types (sorted, unique); empty: automatic
  std::vector<int> active_mapped;            // the model types named by the last type mapping (ahip_compute, ahip_map_types_dev); used when the model has more than 16 types and nothing was set
  unsigned char *slot_dev = nullptr;         // [T] model type -> compact slot, 0xFF = inactive (valid while `active` is non-empty)
  const unsigned char *slot_cur = nullptr;   // slot_dev while a fused kernel is about to run on the subset, else null: what the three writers are handed (run_model_once)
  std::vector<double> rcut_fused_host;       // [A*A] slice of rcut_model_host at active x active
  double *rcut_fused_dev = nullptr;
  long long chunk_edges = 2000000;
  int reserve_wgs = 0;                      // workgroup slots the persistent fused kernels leave free (for kernels of other streams)
  bool timing = false;
  TilePack opt_tile_pack = TilePack::Auto;  // auto | separate | fused (auto = fused up to 262 144 centres per call): tile packing inside the single-pass edge build where the tile shape is known up front, or always by the stand-alone kernels (A/B, tests)
  EdgeSchedule opt_edge_schedule = EdgeSchedule::Auto;   // auto | static | dynamic: unit schedule of the single-pass edge build (edges.hip)
  DenseCentres opt_dense_centres = DenseCentres::Whole;   // whole | split: a list with a few centres above a fused kernel's tile goes to the layer-at-a-time kernels as a whole, or only those centres do (allegro_hip.hip: run_model_once)
  WideTile opt_wide_tile = WideTile::S64;                 // 64 | auto: k_fused_lx on 64-slot tiles only, or on its 128-slot shape when the list's largest degree asks for it (fused_shapes.h: fused_has_wide_tile)
  Lx64MlpWidth opt_lx64_mlp_width = Lx64MlpWidth::W64;    // 64 | auto: k_fused_lx2 (33..64 tensor features) at MLP width <= 64 only, or also on its MLP-width-128 instances for mlp_width 65..128 (fused_shapes.h: the gates' lx64_w128)
  EnvBackward opt_env_backward = EnvBackward::Auto;       // auto | centre | edge: k_fused's transposed environment linear once per centre on tiles of <= 3 centres (f16x2, 4-wave tiles: the instances that have the form; auto and centre are the same rule), or per edge on every tile (fused.hip: FusedArgs::env_bwd; a kernel argument, no state depends on it)
  bool cutoff_strict = false;               // edge kept iff rsq < cut^2 (the KOKKOS reference path) instead of rsq <= cut^2 (the host path)

  // weights
  DeviceWeights<float> wf;
  DeviceWeights<double> wd;
  void *cg_dev = nullptr;                    // AhipCgEntry[ncg_full]
  int ncg_full = 0, ncg_scalar = 0;
  double *rcut_model_dev = nullptr;          // [T*T]

  // neighbor list (device)
  int inum = 0, nall = 0;
  long long nneigh = 0;
  bool have_list = false;
  int max_list_row = -1;                     // longest row of the installed list (-1: unknown, e.g. a caller-owned device list)
  const int *d_ilist = nullptr, *d_nloff = nullptr, *d_nlj = nullptr;   // current (owned or borrowed)
  DevBuf b_ilist, b_nloff, b_nlj;
  std::vector<int> h_flat_j, h_off32, h_ilist;

  // per-call host-path staging
  DevBuf b_x, b_ftype, b_mtype, b_f, b_eatom, b_engvir, b_cutsq, b_flagwork;
  std::vector<int> h_ftype, h_mtype;
  std::vector<double> h_x, h_f, h_eatom, h_cutsq_dev;      // h_cutsq_dev: what b_cutsq currently holds (device path); h_x: page-locked copy of the caller's positions
  std::map<const void *, std::pair<void *, size_t>> pinned;   // host vectors currently page-locked (allegro_hip.hip: pin_host)

  // ahip_compute_cell: rows = atoms then ghosts (positions, model types, forces, per-atom energies), the ghosts' source atoms and shifts, the 7 sums; the
  // ghost count of the last call (first capacity guess of the next) and its sources on the host (ahip_last_cell_rows)
  DevBuf c_x, c_mtype, c_f, c_eatom, c_src, c_shift, c_engvir;
  int cell_nghost_last = 0, cell_natoms = -1;
  std::vector<long long> cell_src_host;
  // ahip_compute_cells (the rows above are then those of the whole batch): the packed upload (positions, structure table, model types, atom -> structure), the
  // rows at their places in the cloud, the 8 sums per structure, and the last batch's ghost counts (ahip_last_cells_ghosts)
  DevBuf c_in, c_xp, c_out;
  int cells_nstruct = -1;
  std::vector<long long> cells_nghost_host;
  // ahip_compute_cell_reuse: what a model holds from one call to the next.  list_serial counts every installation of a neighbor list (allegro_hip.hip:
  // install_list_host, ahip_neigh_update_dev; neigh.hip: neigh_build, neigh_from_table) and every successful ahip_set_option; the hold is valid while its own
  // serial is the model's, so nothing else has to know about it.  On the device: the staged positions of the call, the wrapped atom positions at the hold, the
  // integer image of every ghost, the squared displacements (float32 bit patterns) with their maximum behind them.  The rows, the ghosts' sources and the list
  // are those of ahip_compute_cell above.
  unsigned long long list_serial = 0;
  struct CellHold {
    unsigned long long serial = 0;           // list_serial when the hold was taken; 0: nothing is held
    int natoms = 0, nghost = 0, pbc[3] = {0, 0, 0};
    double skin = 0.0, cell[9] = {0}, images[3] = {0, 0, 0}, min_height = 0.0;      // images: M_d = ceil(rc / h0_d) + 1; min_height: over the periodic axes
    std::vector<int> mtype;
  } hold;
  DevBuf r_xin, r_xhold, r_img, r_disp;
  long long reuse_calls = 0, reuse_rebuilds = 0;
  // ahip_relax_cell (neigh.hip: relax_*): the optimiser's state lives on the device.  Unwrapped positions and velocities in two buffers each (a move reads one
  // pair and writes the other), the fixed-atom mask, per atom [v.F, F.F, v.v] and the float32 bits of |F|^2, and the RelaxState block with the reduced
  // sums and maxima behind it.  The rows, the hold and the displacement bits are those of ahip_compute_cell_reuse above.
  DevBuf q_x[2], q_v[2], q_fixed, q_part, q_fbits, q_state;
  // ahip_relax_vcell: q_x holds the reference coordinates q; besides, per atom G = D^T F, the unwrapped x = D q, and the VcellState block
  DevBuf q_g, q_xc, q_vstate;
  // ahip_md_cell (neigh.hip: md_*): q_x holds the unwrapped positions and q_v the post-thermostat velocity w, as the relaxation holds x and v; besides, the
  // velocity v_n of the configuration whose forces are on the device, the masses, the MdState block, the thermo rows and the frames
  DevBuf q_vnow, q_mass, q_mstate, q_thermo, q_frames;
  // ahip_npt_cell (neigh.hip: npt_*): the buffers of ahip_md_cell, and of its own the NptState block, thermo rows of ten columns and the cell of every frame
  DevBuf q_nstate, q_nthermo, q_fcells;

  // edge list + workspace
  DevBuf b_cnt, b_eoff, b_eii, b_ej, b_rvec, b_partial, b_ws, b_misc;
  DevBuf b_ett;                              // per-edge packed model types (centre << 4 | neighbour), fused path only
  bool have_ett = false;                     // b_ett matches the current edge list (written by the single-pass edge build)
  long long nedges = 0;
  int edges_T_size = 0;                      // sizeof(T) of b_rvec contents
  std::vector<int> h_eoff;
  int last_max_deg = 0;
  std::string last_path;
  // The single-pass edge build (edges.hip) leaves its counters -- edge total, largest degree, number of heavy centres -- on the device and
  // copies them to pinned memory asynchronously; the host waits for that copy (edges_counts) only where it needs one of the values, never on
  // the fused path of a bounded list (no hipStreamSynchronize per ahip_compute_dev* call).
  bool counts_pending = false;               // nedges / last_max_deg / nheavy are not valid yet: call edges_counts()
  long long nedges_hint = 0;                 // edge total of the last read-back that was waited for, else an estimate (heuristics only)
  const int *d_maxdeg = nullptr;             // device word holding the largest degree of the current edge list (single-pass build)
  // tile packing done by the single-pass edge build (edges.hip): requested shape (0 = none), whether the current edge list carries it, its arrays
  int pack_slots = 0, pack_maxa = 0;
  bool tiles_packed = false;
  DevBuf b_tile_a0, b_tile_e0, b_centre, b_ntiles;
  const int *d_ntiles_last = nullptr;        // device word with the tile count of the last fused launch; last_tile_slots: its edge slots per tile (0: chosen on the device from the largest degree)
  int last_tile_slots = 0;

  // Centres with more edges than a tile of the wide fused kernel holds (fused_lx.hip): found by the edge build when
  // heavy_thresh > 0, evaluated by the layer-at-a-time kernels on a compact copy of their edges (hv_*)
  int heavy_thresh = 0, nheavy = 0;
  long long hv_nedges = 0;
  DevBuf hv_eoff, hv_eii, hv_ej, hv_rvec, hv_ilist, hv_engvir;
  // option dense_centres=split behind the two-pass edge build (edges.hip: edges_list_heavy): edge total of the listed centres and the largest degree among the
  // others, read back with the build's own counts; lt_*: the compact copy of the list WITHOUT the listed centres that the fused kernel then runs on
  long long heavy_listed_edges = 0;
  int light_max_deg = 0;
  DevBuf lt_eoff, lt_eii, lt_ej, lt_rvec, lt_ilist;
  // what the last evaluation handed to the layer-at-a-time kernels beside a fused kernel (ahip_last_heavy_centres), and the edges its tiles held when that is
  // not the whole list (-1: it is)
  int last_heavy_centres = 0;
  long long last_heavy_edges = 0, last_tile_edges = -1;

  // `compute allegro`: registered output names and their values from the last host-path compute
  std::vector<std::string> custom_names;
  std::map<std::string, std::vector<double>> custom_out;
  DevBuf b_vatom;                           // "atomic_virial" [nall][9], allocated only while that output is registered

  // timings
  std::vector<TimingSlot> slots;
  std::string timing_names;
  std::vector<double> timing_ms, timing_counts;

  // scratch of the device-wide primitives (scan, column sums): per model, see prims.h
  PrimScratch prim;

  // fused path private state (fused.hip: model S shape; fused_lx.hip / fused_lx2.hip: l_max = 2, 32 / 64 tensor features)
  std::vector<hipEvent_t> f_events;          // host-pointer path: one event per returned chunk of f (allegro_hip.hip: ahip_compute)
  int *h_alarm = nullptr;                    // page-locked, device-mapped word raised by the f16x2 instances of the fused kernels (fused_h.h): see alarm_word()
  FusedState *fused_state = nullptr;
  FusedLxState *fusedlx_state = nullptr;
  FusedLxState *fusedlx2_state = nullptr;    // wave-pair version of the 64-feature shape (fused_lx2.hip)

  // neighbor builder state
  void *nb_state = nullptr;
  // single-pass edge build state (edges.hip)
  void *edge_state = nullptr;
};

// ---- stage timing ------------------------------------------------------------------------------
void timing_drain(Model &m, TimingSlot &t, size_t keep);          // allegro_hip.hip: reads pairs until at most `keep` are outstanding (waits for them)
struct StageTimer {
  Model &m; hipStream_t s; int idx = -1; hipEvent_t eb = nullptr;
  StageTimer(Model &m_, const char *name, hipStream_t s_) : m(m_), s(s_) {
    if (!m.timing) return;
    for (size_t i = 0; i < m.slots.size(); ++i) if (m.slots[i].name == name) idx = (int)i;
    if (idx < 0) { TimingSlot t; t.name = name; m.slots.push_back(t); idx = (int)m.slots.size() - 1; }
    TimingSlot &t = m.slots[idx];
    if (t.head - t.tail >= TIMING_RING) timing_drain(m, t, TIMING_RING / 2);
    const size_t k = t.head % TIMING_RING;
    if (k >= t.ring.size()) {
      std::pair<hipEvent_t, hipEvent_t> e{nullptr, nullptr};
      AHIP_CHECK(hipEventCreate(&e.first)); AHIP_CHECK(hipEventCreate(&e.second));
      t.ring.push_back(e);
    }
    eb = t.ring[k].second;
    AHIP_CHECK(hipEventRecord(t.ring[k].first, s));
  }
  ~StageTimer() { if (idx >= 0) { (void)hipEventRecord(eb, s); ++m.slots[idx].head; } }
};

// ---- generic path (generic_engine.h via allegro_hip.hip) -------------------------------
struct ComputeArgs {
  int nlocal, nghost;
  const double *x;          // device [nall][3]
  const int *ftype;         // device [nall], index into cutsq
  const double *cutsq;      // device [nft*nft]
  int nft;
  const int *mtype;         // device [nall] model types
  double *f;                // device [nall][3], accumulated
  double *eatom;            // device [nall] or null
  double *engvir;           // device [7]
  hipStream_t stream;
  double *vatom = nullptr;  // device [nall][9] or null: per-atom virial W_j[a][b] = -sum over edges e with NEIGHBOUR j of r_e[a] g_e[b] (output "atomic_virial"), accumulated
};

// ---- fused path entry points (fused.hip; the host-emulation test build links a stub) ---------
// Returns true when the fused MFMA kernels support this model shape at all.
bool fused_model_supported(const Model &m, std::string *why);
// Runs forward+backward for all centres; edges already built (b_eoff/b_eii/b_ej/b_rvec as float).
// Returns false (and sets *why) if this particular list cannot be handled (e.g. too many edges per atom).
bool fused_run(Model &m, const ComputeArgs &a, std::string *why);
void fused_free(Model &m);
// Tile shapes (edge slots, centres) the single-pass edge build packs for (allegro_hip.hip: run_model_once); the kernel files static_assert their own shapes against them
inline constexpr int FUSED_TILE_SLOTS = 64, FUSED_TILE_MAXA = 6;     // k_fused, 4-wave tiles
inline constexpr int FUSED_MAX_TILE_SLOTS = 128;                     // k_fused, 8-wave tiles: the edge count above which a centre is "heavy" for it (option dense_centres=split)
inline constexpr int LX_TILE_SLOTS = lx_tile_slots(false), LX_TILE_MAXA = lx_tile_maxa(false);      // k_fused_lx2 and the 4-wave shape of k_fused_lx (fused_shapes.h); the largest shape a model may run on: lx_max_tile_slots below
// f16x2 arithmetic (fused_h.h): device address of the model's alarm word (allocated on first use); fused_poll_alarm throws StateError when a kernel has
// raised it -- the host-pointer call polls behind its own synchronisation, device-resident callers meet it at their next evaluation
int *alarm_word(Model &m);
bool alarm_take(Model &m);                  // true (and cleared) when a kernel has raised the word since the last call
void fused_poll_alarm(Model &m);            // alarm_take + the policy: auto -> degrade to f32 and report once; explicit f16x2 -> StateError
// the model at the fixed shape of the fused kernel family its l_max and tensor features belong to (fused_shapes.h: the model itself when it is exactly that shape,
// else zero-padded, and an l_max = 1 model with more than 32 tensor features lifted to l_max = 2)
// ... of the model restricted to its active types when a subset is in force (Model::active)
inline const HostModel &fused_host_model(Model &m) {
  const HostModel &h = m.hm;
  const FusedFamily cls = fused_shape_class(h);
  const int WF = fused_WF(h);                // hidden width of the latent MLP: 64, or 128 for a model with mlp_width 65..128 (fused_shapes.h; a model of 33..64 tensor features
                                             // gets here with such a width under option lx64_mlp_width=auto only: without it the wide gate refuses the model and nothing pads it)
  const int RF = fused_RF(h);                // width of the read-out MLP: 32, or 64 for a model with readout_width 33..64
  if (m.active.empty() && fused_shape_exact(h, cls, WF, RF)) return h;
  if (!m.hm_fused_ready) {
    m.hm_fused = m.active.empty() ? fused_shaped_model(h, cls, WF, RF) : fused_shaped_model(subset_host_model(h, m.active), cls, WF, RF);
    m.hm_fused_ready = true;
  }
  return m.hm_fused;
}
// what the fused side reads in place of num_types / rcut_model_*: the active count for the gates (-1: every type), the cutoffs at active x active
inline int fused_n_active(const Model &m) { return m.active.empty() ? -1 : (int)m.active.size(); }
inline const std::vector<double> &fused_rcut_host(const Model &m) { return m.active.empty() ? m.rcut_model_host : m.rcut_fused_host; }
inline const double *fused_rcut_dev(const Model &m) { return m.active.empty() ? m.rcut_model_dev : m.rcut_fused_dev; }
// host-mapped word next to the f16x2 alarm word (alarm_word(m) + 1): 1 + the model type of an atom whose type is not in the active set, raised by the writers
// of fused-side types (such an atom takes slot 0, so every index stays in range); inactive_take reads and clears it, fused_poll_alarm reports it as ArgError
inline int *inactive_word(Model &m) { return alarm_word(m) + 1; }
int inactive_take(Model &m);
// the arithmetic policy (arith_policy.h) applied to a model: k_fused (wide = false) or the wide kernels
inline bool arith_may_degrade(const Model &m) { return arith_may_degrade(m.arith); }
inline bool fused_tb_is_table(const Model &m) { return fused_tb_is_table(m.opt_fused_tb); }
inline bool fused_lx64_w128(const Model &m) { return m.opt_lx64_mlp_width == Model::Lx64MlpWidth::Auto; }      // the gates' trailing argument (fused_shapes.h)
inline Arith resolve_arith(const Model &m, bool wide) {
  return resolve_arith(arith_effective(m.arith.opt), m.hm.allow_tf32 != 0, m.arith.degraded, m.arith.force_f32, fused_tb_is_table(m), wide);
}
// Edge slots of the largest tile the wide kernel of family `fam` may use for this model: the edge count above which a centre is "heavy" (listed by the edge build,
// skipped by the kernel, evaluated by heavy_generic) and against which the one-in-eight give-up rule counts.  128 under option wide_tile=auto where the 8-wave shape
// of k_fused_lx exists for the model's arithmetic and depths, else 64.
inline int lx_max_tile_slots(const Model &m, FusedFamily fam) {
  return lx_tile_slots(m.opt_wide_tile == Model::WideTile::Auto && fused_has_wide_tile(fam, resolve_arith(m, true), m.hm.mlp_depth, m.hm.readout_depth, fused_WF(m.hm), fused_RF(m.hm)));
}
// the model computes in float64 (option precision, or the model file's own dtype): layer-at-a-time kernels only
inline bool model_runs_f64(const Model &m) { return m.opt_precision == Model::Precision::Float64 || m.hm.is_f64(); }
// thrown by a fused kernel's prepare step when fused_arith=auto meets a model the f16x2 split cannot carry; run_model degrades the model and dispatches again
struct ArithDegraded {
  std::string why;
};
// range findings of append_frag_h (fused_h.h) over a model's weight stream
enum { H_RANGE_OVERFLOW = 1, H_RANGE_TINY = 2 };
// H_RANGE_TINY over a whole model: any [K][N] block of a dense-layer tensor whose largest weight is non-zero and below 2^-10 (fused_lx2.hip lays its stream
// out in sub-blocks of the matrices and asks here instead of per block)
inline int model_tiny_linear(const HostModel &h) {
  for (const auto &kv : h.tensors) {
    const HostTensor &t = kv.second;
    const std::string &n = kv.first;
    const bool dense = n.find(".lat.w") != std::string::npos || n.find(".env") != std::string::npos || n.find(".mix") != std::string::npos || n == "emb.w" || n == "out.w0" ||
                       (n == "out.w1" && h.readout_depth == 2) || (n.rfind("tb.w", 0) == 0);      // (out.w1 of a depth-1 read-out is the final 32 -> 1 vector, read in float32)
    if (!dense || t.shape.size() < 2) continue;
    const long long blk = (long long)t.shape[t.shape.size() - 2] * t.shape[t.shape.size() - 1], nb = blk > 0 ? t.numel() / blk : 0;
    for (long long b = 0; b < nb; ++b) {
      double wmax = 0.0;
      for (long long i = 0; i < blk; ++i) wmax = std::max(wmax, std::fabs(t.data[(size_t)(b * blk + i)]));
      if (wmax > 0.0 && wmax < 0x1p-10) return H_RANGE_TINY;
    }
  }
  return 0;
}
// what a prepare step does with them: explicit f16x2 -> the overflow is an error (the tiny linear is the caller's choice); auto -> ArithDegraded
inline void arith_range_verdict(const Model &m, int flags) {
  if (!flags) return;
  const char *what = (flags & H_RANGE_OVERFLOW) ? "a weight of this model exceeds float16's range" : "a linear of this model has all its weights below 2^-10 (float16 subnormal territory for the split)";
  if (arith_may_degrade(m)) throw ArithDegraded{what};
  if (flags & H_RANGE_OVERFLOW) throw UnsupportedError(std::string("fused_arith=f16x2: ") + what + "; use fused_arith=f32 (or auto)");
}
// f16x2 arithmetic: the backward pass is linear in its upstream gradient scale[type] / sqrt(avg_num_neighbors) and runs scaled by the power of two that brings that
// gradient into [0.5, 1) -- PER CENTRE TYPE since round 6 (the kernels derive it from scale[t_i] with frexp: energy scales that differ by orders of magnitude
// between species each get their own; one global power of two from the largest left the small species in float16's subnormals)
// the same for the wide shapes (l_max = 2): 32 tensor features on k_fused_lx (fused_lx.hip), 64 on the wave-pair kernel k_fused_lx2 (fused_lx2.hip:
// two waves per SIMD, each wave half of the channels); fusedlx_free releases the states of both
bool fusedlx_model_supported(const Model &m, std::string *why);
bool fusedlx_run(Model &m, const ComputeArgs &a, std::string *why);
bool fusedlx2_run(Model &m, const ComputeArgs &a, std::string *why);
void fusedlx_free(Model &m);

// ---- single-pass float32 edge build (edges.hip; the host-emulation build links a stub returning false) ----
// Fills m.nedges, m.last_max_deg, b_eoff/b_eii/b_ej/b_rvec exactly like build_edges<float>; false = a list
// row is too long for the register-resident version and the caller must run the two-pass kernels.
bool edges_build_f32(Model &m, const ComputeArgs &a);
// waits for the counters of the last edges_build_f32 if they are still in flight (m.counts_pending) and installs them in m
// Synchronous copies between PAGEABLE host memory and the device, staged through the library's own page-locked buffer.  Handed a pageable pointer, the
// HIP runtime pins the range on the fly for copies above 1 MiB and caches that pinning by address; in a long-lived process the heap hands pages back to the
// system and gets them back later (malloc trimming), the cached pinning then points at nothing, and the copy engine faults on a HOST address -- seen as an
// intermittent "Memory access fault by GPU ... on address 0x5555..." during the weight upload of the n-th model of a process (round 4, tests -m gpu:
// 4 of 10 full runs).  Page-locked memory of our own never takes that path.
void copy_h2d(void *dst_dev, const void *src_host, size_t bytes);
void copy_d2h(void *dst_host, const void *src_dev, size_t bytes);
void edges_counts(Model &m);
// longest row of a device-resident CSR list (list hand-over only: one small kernel + a 4-byte read-back)
int edges_max_row(Model &m, int inum, const int *offsets_dev);
void edges_free(Model &m);
// compact copy (m.hv_*) of the edges of the m.nheavy centres the last edges_build_f32 listed
void edges_compact_heavy(Model &m, const ComputeArgs &a);
// Option dense_centres=split on the two-pass route (generic_engine.h: build_edges).  edges_list_heavy enqueues, behind the scan of the edge counts, the kernel that
// lists the centres with more than `thresh` edges -- ascending, into the buffers and header words the single-pass build fills -- and the copy of its counts;
// edges_list_heavy_counts installs them (heavy_thresh, nheavy, heavy_listed_edges, light_max_deg) once build_edges has waited for its own read-back.
// edges_compact_light: compact copy (m.lt_*) of the list without those centres.  (Not in the host-emulation build: no fused kernel there.)
void edges_list_heavy(Model &m, const ComputeArgs &a, int thresh);
void edges_list_heavy_counts(Model &m, int thresh);
void edges_compact_light(Model &m, const ComputeArgs &a);

// ---- float32 dense layers of the generic path on the matrix cores (gemm.hip; the host-emulation build links a stub
// returning false and keeps the one-thread-per-output kernels) ----
// C[e][n] (+)= sum_k A[e][k] * (transB ? W[n][k] : W[k][n])
bool gemm_f32(hipStream_t s, long long E, int K, int N, const float *A, int lda, const float *W, int ldw, bool transB, float *C,
              int ldc, bool accumulate, float *silu_out = nullptr, const float *dsilu_z = nullptr);
// wave-per-row versions of k_latent_update_bwd / k_embed_bwd_Y (same stubs in the emulation build)
bool latent_update_bwd_f32(hipStream_t s, long long E, int S, const float *dx, const float *u, const float *fc, const float *res,
                           float *du, float *dfc, float *dxprev);
bool embed_bwd_Y_f32(hipStream_t s, long long E, int D, int U, const float *dV, const float *w, float *dY);
bool env_bwd_Y_f32(hipStream_t s, long long E, int D, int U, const float *denv, const int *e_ii, int c0, const float *om, float *dY);
// tensor product with the CG table unrolled at compile time (l_max 1, 2); scalar_only = last layer (l3 = 0 outputs)
bool tp_fwd_f32(hipStream_t s, long long E, int L, bool scalar_only, int U, const float *pw, const float *V, const float *env,
                const int *e_ii, int c0, float *Vp);
bool tp_bwd_f32(hipStream_t s, long long E, int L, bool scalar_only, int U, const float *pw, const float *V, const float *env,
                const int *e_ii, int c0, const float *dVp, float *dV, float *denv_e);

// ---- neighbor builder (neigh.hip; stubbed in the host-emulation build) -------------------------
void neigh_build(Model &m, int nlocal, int nall, const double *x_dev, const double *lo, const double *hi,
                 double rc_list, hipStream_t s);
void neigh_from_table(Model &m, int inum, int nall, const int *ilist_dev, const int *numneigh_dev, const int *table_dev,
                      long long stride_atom, long long stride_slot, int mask, hipStream_t s);
void map_types(Model &m, int n, const int *type_dev, int ntypes, const int *mapper_host, int *out_dev, hipStream_t s);
void neigh_free(Model &m);
// periodic images of a single rank's own atoms inside the halo (neigh.hip); returns their number (may exceed `capacity`: then the arrays hold the first `capacity`)
int borders_local(Model &m, int nlocal, const double *x, const int *mtype, const double *lo, const double *hi, const double *box, double rc, int capacity,
                  double *xg, int *mtg, long long *src, double *shift, hipStream_t s);
// any periodic cell (neigh.hip; cell: row-major double[9], rows = lattice vectors; pbc: int[3]).  wrap_cell: one launch, no synchronisation.  borders_cell: the
// images n != 0 of the rank's own atoms with -rc / h_d <= s_d + n_d < 1 + rc / h_d on every periodic axis, same output contract as borders_local.
// cell_bounding_box: the eight corners of the cell, widened by `margin`.  All three throw ArgError for a singular or non-finite cell, before any launch.
void wrap_cell(Model &m, int n, double *x, const double *cell, const int *pbc, hipStream_t s);
int borders_cell(Model &m, int nlocal, const double *x, const int *mtype, const double *cell, const int *pbc, double rc, int capacity,
                 double *xg, int *mtg, long long *src, double *shift, hipStream_t s);
void cell_bounding_box(const double *cell, double margin, double *lo, double *hi);
// The held list of ahip_compute_cell_reuse (neigh.hip; criterion and proof: include/allegro_hip.h).  cell_hold_take, behind a rebuild whose rows are in m.c_x /
// m.c_src / m.c_shift: copies the wrapped atom rows, recovers every ghost's integer image n = round(shift . cell^-1) and fills m.hold (enqueues on `s`, no
// synchronisation; the caller sets the serial).  cell_hold_refresh: ArgError for a singular or non-finite `cell` before any launch; false, without a launch,
// when the change of the cell alone fails the criterion; else uploads x, rewrites every row of m.c_x as the exact image in `cell` of the new position
// (k_cell_refresh), reads the largest displacement back (one synchronisation) and says whether the held list still holds every pair within the cutoffs.
void cell_hold_take(Model &m, int natoms, int nghost, const double *cell, const int *pbc, double skin, double rc, hipStream_t s);
bool cell_hold_refresh(Model &m, const double *x_host, const double *cell, hipStream_t s);
// FIRE on the device (ahip_relax_cell; algorithm: include/allegro_hip.h).  RelaxState is the block the host reads back every check_every moves; k_relax_decide
// is its only writer on the device.  relax_begin uploads the start (never wrapped), zeroes the velocities and writes the initial state; relax_rows_fresh says
// that the rows of m.c_x were just rebuilt from the current positions (displacements 0); relax_step enqueues gather, the two reductions, decide and move for
// the move whose input buffers are `in` (0 or 1) -- no wait; relax_read waits for the stream and returns the state; relax_resume sets the status back to RUNNING.
// The positions that count after a read are q_x[state.moves & 1].
enum { RELAX_RUNNING = 0, RELAX_CONVERGED = 1, RELAX_NEED_REBUILD = 2, RELAX_NONFINITE = 3 };
struct RelaxFire {
  double fmax, dt_max, max_step, f_inc, f_dec, alpha_start, f_alpha, skin;
  int n_min;
};
struct RelaxState {
  double dt, alpha, c1, c2, s;       // s: the factor min(1, max_step / |dr|) of the last move
  double fmax2, u2;                  // what the last decision saw: max |F_i|^2 and U^2 (float32 values)
  double sums[3];                    // v.F, F.F, v.v (prim_sum_columns_f64)
  int npos, status, moves;
  int fbits, ubits;                  // prim_max_i32 of the |F_i|^2 and displacement bit patterns
  int pad;
};
void relax_begin(Model &m, int natoms, const double *x_host, const int *fixed_host, double dt_start, double alpha_start, hipStream_t s);
void relax_rows_fresh(Model &m, int natoms, hipStream_t s);
void relax_step(Model &m, int in, const RelaxFire &p, hipStream_t s);
RelaxState relax_read(Model &m, hipStream_t s);
void relax_resume(Model &m, hipStream_t s);
// FIRE over the atoms and the cell (ahip_relax_vcell; algorithm: include/allegro_hip.h).  The fixed-cell kernels and RelaxState above are not touched: the
// variable cell has a state block of its own, which also carries what the host cannot hand over by value because it does not look between moves -- the
// deformation gradient D with its velocity, the start cell A0, the hold (cell, M_d, min h0) the reuse criterion is taken against, and the geometry of the current
// cell A0 D^T.  k_vcell_decide is its only writer on the device; the host writes it at the start and behind a rebuild (vcell_held), with the stream idle.
// vcell_step: gather, reductions, decide, move for the move whose input buffers are `in`; vcell_check: gather, reductions and the decisions 1-4 without a move,
// for the configuration the last move of a run left.  vcell_positions forms the unwrapped x = D q of buffer `in` in m.q_xc (device).
struct VcellPar {
  RelaxFire fire;
  double smax, pressure, cfac;       // cfac: the factor c of the strain rows, > 0
  int hydrostatic, mask[6];          // mask: xx, yy, zz, xy, xz, yz
  int check_only;
};
struct VcellState {
  double dt, alpha, c1, c2, s;
  double fmax2, u2, sext, detD;      // what the last decision saw: max |F_i|^2, U^2 (float32 values), max |W_ext,ab| / V; det D of the current cell
  double sums[3];                    // v.G, G.G, v.v over the atom rows (prim_sum_columns_f64); the decision adds the strain rows
  double D[9], vD[9];                // row-major; x = D q, a_d = D a0_d
  double A0[9];
  double hold_cell[9], hold_images[3], hold_min_height;
  CellGeom geom;                     // of the current cell: h = A0 D^T, inv; pbc all set
  int npos, status, moves;
  int fbits, ubits;
  int pad;
};
void vcell_begin(Model &m, int natoms, const double *x_host, const int *fixed_host, const double *cell, double dt_start, double alpha_start, hipStream_t s);
void vcell_step(Model &m, int in, const VcellPar &p, hipStream_t s);
void vcell_check(Model &m, int in, const VcellPar &p, hipStream_t s);
void vcell_positions(Model &m, int natoms, int in, hipStream_t s);
VcellState vcell_read(Model &m, hipStream_t s);
void vcell_held(Model &m, VcellState st, hipStream_t s);
void vcell_resume(Model &m, hipStream_t s);
// MD on the device (ahip_md_cell; algorithm: include/allegro_hip.h).  BAOAB over the held rows with the buffers, the row writer and the rebuild decision of the
// relaxation, whose kernels and state blocks are not touched.  MdState is the block the host reads back every check_every steps; k_md_decide is its only writer
// on the device.  md_begin uploads the start (never wrapped), w = v, the masses and the mask, and sizes the thermo rows and the frames; md_step enqueues gather,
// the reductions and decide for the configuration whose buffers are `in` (0 or 1), and with `move` the move into the other pair -- no wait; md_read waits for the
// stream and returns the state; md_resume sets the status back to RUNNING.  The positions that count after a read are q_x[state.n & 1].  md_noise: xi of atoms
// 0 .. n-1 at one step, by the device function the move uses.
enum { MD_RUNNING = 0, MD_DONE = 1, MD_NEED_REBUILD = 2, MD_NONFINITE = 3 };
struct MdPar {
  double dt, hdtf, c1, c2, gamma, kT, mvv2e, skin;      // hdtf = 0.5 dt ftm2v; c1 = exp(-gamma dt); c2 = sqrt(1 - c1^2)
  unsigned long long seed, step0;
  int nsteps, sample_every, frame_every;
};
struct MdState {
  double u2, fmax2;                  // what the last decision saw: U^2 and max |F_i|^2 (float32 values)
  double sums[1];                    // sum_i m_i |v_i|^2 (prim_sum_columns_f64)
  int status, n;                     // n: the configuration whose forces are on the device, 0 .. nsteps
  int fbits, ubits;                  // prim_max_i32 of the |F_i|^2 and displacement bit patterns
};
void md_begin(Model &m, int natoms, const double *x_host, const double *v_host, const double *mass_host, const int *fixed_host, size_t thermo_rows, size_t frame_rows,
              hipStream_t s);
void md_step(Model &m, int in, const MdPar &p, bool move, hipStream_t s);
MdState md_read(Model &m, hipStream_t s);
void md_resume(Model &m, hipStream_t s);
void md_noise(unsigned long long seed, unsigned long long step, int n, double *out_dev, hipStream_t s);
// MD at constant pressure on the device (ahip_npt_cell; algorithm: include/allegro_hip.h).  The BAOAB of ahip_md_cell inside an isotropic stochastic cell
// rescaling, with the cell handling of ahip_relax_vcell; the kernels and state blocks of both are not touched.  NptState carries what MdState carries and,
// because the host does not look between steps, the current cell with its geometry, the factor mu of the last rescaling, the hold (cell, M_d, min h0) the reuse
// criterion is taken against, and V and P of the last decision.  k_npt_decide is its only writer on the device; the host writes it at the start and behind a
// rebuild (npt_held), with the stream idle.  npt_begin: md_begin, the thermo rows of ten columns, the frame cells and the state block in `cell`; npt_step, npt_read,
// npt_resume: as md_step, md_read, md_resume.  The positions that count after a read are q_x[state.n & 1], in the cell state.geom.h.  npt_noise: xi_V of one step.
struct NptPar {
  MdPar md;
  double p0, beta_over_tau, noise;   // noise = sqrt(2 kT beta_T dt / tau_p): xi_V is scaled by noise / sqrt(V); 0 = no random number is drawn
};
struct NptState {
  double u2, fmax2;                  // what the last decision saw: U^2 and max |F_i|^2 (float32 values)
  double sums[1];                    // sum_i m_i |v_i|^2 (prim_sum_columns_f64)
  double mu, V, P;                   // the factor of the last rescaling (1 before the first); volume and pressure of the last decision
  double hold_cell[9], hold_images[3], hold_min_height;
  CellGeom geom;                     // of the current cell; pbc all set
  int status, n;                     // the statuses of MdState; n: the configuration whose forces are on the device, 0 .. nsteps
  int fbits, ubits;
};
void npt_begin(Model &m, int natoms, const double *x_host, const double *v_host, const double *mass_host, const int *fixed_host, const double *cell, size_t thermo_rows,
               size_t frame_rows, hipStream_t s);
void npt_step(Model &m, int in, const NptPar &p, bool move, hipStream_t s);
NptState npt_read(Model &m, hipStream_t s);
void npt_held(Model &m, NptState st, hipStream_t s);
void npt_resume(Model &m, hipStream_t s);
void npt_noise(unsigned long long seed, unsigned long long step, double *out_dev, hipStream_t s);
// A batch of cells as one non-periodic cloud (neigh.hip).  cells_plan is host-only and throws ArgError before any launch: per structure the geometry (a singular
// or non-finite cell names its index), the 32-bit bound on atoms + images, the extent of its rows -- the Cartesian bounding box of its parallelepiped with the
// fractional range [-m_d, 1 + m_d] on periodic axes and the range its atoms have on open ones -- and its origin: uniform slots of the largest extent plus
// rc + 1e-6 on a near-cubic grid, so that no row of one structure is within rc + 1e-6 of a row of another.  `table` receives nstruct + 1 device-layout
// entries (returns the size of one); lo / hi the bounding box of all slots, and more than 2^26 bins of neigh_build's grid over it is the "split the batch" error.
// The others enqueue on `s`: wrap (k_cell_wrap per structure, out of place), count + ONE scan over the batch (returns the ghost total: the one
// synchronisation), fill (the rows borders_cell gives for each structure alone, src + first[s]), place (own frame + origin), reduce (out[8 s]: energy, virial
// xx yy zz xy xz yz from the row sum of x (x) f before the ghost forces go home, ghost count).
size_t cells_plan(int nstruct, const int *first, const double *x, const double *cells, const int *pbc, double rc, std::vector<unsigned char> &table, double *lo,
                  double *hi);
void cells_wrap(int natoms, const double *xin, const int *mtin, const int *sidx, const void *table, double *x, int *mt, hipStream_t s);
int cells_count(Model &m, int natoms, const double *x, const int *sidx, const void *table, hipStream_t s);
void cells_fill(Model &m, int natoms, int nghost, const double *x, const int *mtype, const int *sidx, const void *table, double *xg, int *mtg, long long *src,
                double *shift, hipStream_t s);
void cells_place(int natoms, int nall, const double *x, const int *sidx, const long long *src, const void *table, double *xp, hipStream_t s);
void cells_reduce(Model &m, int nstruct, int natoms, const void *table, const double *x, const double *f, const double *eatom, double *out, hipStream_t s);
// one rank, ghost g (row nlocal + g) an image of local row src[g]: f[src[g]] += f[nlocal + g] (comm.hip: the reverse exchange of the local plan)
void comm_scatter_local(int nghost, int nlocal, const long long *src, double *f, hipStream_t s);
void nve_first_step(Model &m, int n, int nall, double *x, double *v, double *f, const int *mtype, const double *mass_host, int ntypes, double dt, double ftm2v,
                    hipStream_t s);
void nve_step(Model &m, int mode, int n, double *x, double *v, const double *f, const int *mtype, const double *mass_dev_or_host,
              int ntypes, double dt, double ftm2v, hipStream_t s);

}  // namespace ahip

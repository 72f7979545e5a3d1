// liballegro_hip.so -- C-ABI implementation (include/allegro_hip.h).
//
// Host orchestration of one force evaluation = PairNequIPAllegro<false>::compute
// (/root/reference/pair_nequip_allegro.cpp:333-407): list ingestion, cutoff filter + edge build,
// model forward/backward (generic or fused kernels), force/energy/virial read-out.
// No libtorch, no Kokkos, no CPU fallback: every compute entry point needs a HIP device.
#include "../../include/allegro_hip.h"

#include <pthread.h>
#include <sched.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "engine.h"
#include "generic_engine.h"
#include "cell_geom.h"

using namespace ahip;

struct ahip_model : public ahip::Model {};

static thread_local std::string g_err;

const char *ahip_last_error(void) { return g_err.c_str(); }
namespace ahip {
void set_error(const std::string &s) { g_err = s; }          // comm.hip
std::atomic<int> g_models_alive{0};                          // edges.hip: unit schedule of the edge build
}

template <typename F> static int guarded(F &&fn) {
  try {
    g_err.clear();
    fn();
    return AHIP_OK;
  } catch (const ArgError &e) { g_err = e.what(); return AHIP_ERR_ARG; }
  catch (const StateError &e) { g_err = e.what(); return AHIP_ERR_STATE; }
  catch (const UnsupportedError &e) { g_err = e.what(); return AHIP_ERR_UNSUPPORTED; }
  catch (const HipError &e) { g_err = e.what(); return AHIP_ERR_DEVICE; }
  catch (const std::bad_alloc &) { g_err = "out of host memory"; return AHIP_ERR_DEVICE; }
  catch (const std::exception &e) { g_err = e.what(); return AHIP_ERR_FILE; }
}

int ahip_device_count(int *count) {
  return guarded([&] {
    if (!count) throw ArgError("ahip_device_count: count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { (void)hipGetLastError(); n = 0; }
    *count = n;
  });
}

static void require_model(const ahip_model *m) { if (!m) throw ArgError("model handle is NULL"); }

static void validate_shape(const HostModel &h) {
  if (h.l_max < 0 || h.l_max > 3) throw UnsupportedError("l_max must be 0 .. 3 (got " + std::to_string(h.l_max) + ")");      // 3: layer-at-a-time kernels only
  if (h.num_layers < 1) throw UnsupportedError("num_layers must be >= 1");
  if (h.num_bessels < 1 || h.S < 1 || h.U < 1 || h.mlp_width < 1) throw UnsupportedError("bad model dimensions");
  if (h.mlp_depth < 0 || h.readout_depth < 0) throw UnsupportedError("bad MLP depth");
  if (h.poly_p < 2) throw UnsupportedError("polynomial_cutoff_p must be >= 2");
  if (!(h.r_max > 0)) throw UnsupportedError("r_max must be positive");
  // every tensor must be present with the documented shape
  const int T = h.num_types, B = h.num_bessels, S = h.S, U = h.U, L = h.l_max, W = h.mlp_width, R = h.readout_width;
  auto need = [&](const std::string &n, std::vector<int> shape) {
    const HostTensor &t = h.get(n);
    if (t.shape != shape) throw std::runtime_error("model file: tensor '" + n + "' has unexpected shape");
  };
  auto need_mlp = [&](const std::string &pre, int din, int depth, int width, int dout) {
    std::vector<int> dims{din};
    for (int k = 0; k < depth; ++k) dims.push_back(width);
    dims.push_back(dout);
    for (size_t k = 0; k + 1 < dims.size(); ++k) need(pre + ".w" + std::to_string(k), {dims[k], dims[k + 1]});
  };
  const int npf = L == 0 ? AHIP_CG_L0_NPATHS : (L == 1 ? AHIP_CG_L1_NPATHS : (L == 2 ? AHIP_CG_L2_NPATHS : AHIP_CG_L3_NPATHS));
  const int nps = L == 0 ? AHIP_CG_L0_NPATHS_SCALAR : (L == 1 ? AHIP_CG_L1_NPATHS_SCALAR : (L == 2 ? AHIP_CG_L2_NPATHS_SCALAR : AHIP_CG_L3_NPATHS_SCALAR));
  need_mlp("tb", 2 * T + B, h.mlp_depth, W, S);
  need("emb.w", {S, U * (L + 1)});
  for (int k = 1; k <= h.num_layers; ++k) {
    const std::string lk = "l" + std::to_string(k);
    need(lk + ".env", {S, U * (L + 1)});
    need(lk + ".tp", {k == h.num_layers ? nps : npf, U});
    need_mlp(lk + ".lat", S + U, h.mlp_depth, W, S);
    need(lk + ".res", {2});
    if (k < h.num_layers) need(lk + ".mix", {L + 1, U, U});
  }
  need_mlp("out", S, h.readout_depth, R, 1);
  need("scale", {T});
  need("shift", {T});
}

int ahip_model_load(const char *path, int device, ahip_model **out) {
  return guarded([&] {
    if (!path || !out) throw ArgError("ahip_model_load: NULL argument");
    *out = nullptr;
    HostModel hm = load_model_file(path);                  // throws runtime_error -> AHIP_ERR_FILE
    validate_shape(hm);
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
      (void)hipGetLastError();
      throw HipError("no HIP device visible: allegro-hip has no CPU fallback (hipGetDeviceCount failed or returned 0)");
    }
    if (device < 0 || device >= n)
      throw ArgError("pair_allegro: mismatch between number of ranks and number of available GPUs (device " +
                     std::to_string(device) + " of " + std::to_string(n) + ")");
    AHIP_CHECK(hipSetDevice(device));
    ahip_model *m = new ahip_model();
    try {
      m->hm = std::move(hm);
      m->device = device;
      m->D = (m->hm.l_max + 1) * (m->hm.l_max + 1);
      m->Ka = 2 * m->hm.num_types + m->hm.num_bessels;
      const int T = m->hm.num_types;
      m->rcut_model_host.assign((size_t)T * T, m->hm.r_max);
      if (!m->hm.per_edge_type_cutoff.empty()) m->rcut_model_host = m->hm.per_edge_type_cutoff;
      AHIP_CHECK(hipMalloc((void **)&m->rcut_model_dev, (size_t)T * T * sizeof(double)));
      AHIP_CHECK(hipMemcpy(m->rcut_model_dev, m->rcut_model_host.data(), (size_t)T * T * sizeof(double), hipMemcpyHostToDevice));
      const int lm_ = m->hm.l_max;
      const AhipCgEntry *tab = lm_ == 0 ? ahip_cg_l0 : (lm_ == 1 ? ahip_cg_l1 : (lm_ == 2 ? ahip_cg_l2 : ahip_cg_l3));
      m->ncg_full = lm_ == 0 ? AHIP_CG_L0_N : (lm_ == 1 ? AHIP_CG_L1_N : (lm_ == 2 ? AHIP_CG_L2_N : AHIP_CG_L3_N));
      m->ncg_scalar = lm_ == 0 ? AHIP_CG_L0_NSCALAR : (lm_ == 1 ? AHIP_CG_L1_NSCALAR : (lm_ == 2 ? AHIP_CG_L2_NSCALAR : AHIP_CG_L3_NSCALAR));
      AHIP_CHECK(hipMalloc(&m->cg_dev, (size_t)m->ncg_full * sizeof(AhipCgEntry)));
      AHIP_CHECK(hipMemcpy(m->cg_dev, tab, (size_t)m->ncg_full * sizeof(AhipCgEntry), hipMemcpyHostToDevice));
    } catch (...) { ahip_model_free(m); throw; }
    *out = m;
    m->counted = true;
    g_models_alive.fetch_add(1);
  });
}

namespace ahip {
int *alarm_word(Model &m) {
  if (!m.h_alarm) {
    AHIP_CHECK(hipHostMalloc((void **)&m.h_alarm, 64, hipHostMallocMapped));
    m.h_alarm[0] = 0; m.h_alarm[1] = 0;          // [0] the f16x2 alarm, [1] the inactive-type word (engine.h: inactive_word)
  }
  int *d = nullptr;
  AHIP_CHECK(hipHostGetDevicePointer((void **)&d, m.h_alarm, 0));
  return d;
}
bool alarm_take(Model &m) {
  if (m.h_alarm && *(volatile int *)m.h_alarm != 0) { *m.h_alarm = 0; return true; }
  return false;
}
int inactive_take(Model &m) {
  if (!m.h_alarm) return 0;
  const int v = ((volatile int *)m.h_alarm)[1];
  if (v != 0) m.h_alarm[1] = 0;
  return v;
}
// every fused kernel state of the model (weight streams are rebuilt on the next compute)
static void free_fused_states(Model &m) { fused_free(m); fusedlx_free(m); }
// the report of the inactive-type word (raised = 1 + model type): `when` says which evaluation
static std::string inactive_message(const Model &m, int raised, const char *when) {
  const int mt = raised - 1;
  const std::string name = mt >= 0 && mt < (int)m.hm.type_names.size() ? " (" + m.hm.type_names[(size_t)mt] + ")" : "";
  return std::string("an atom of model type ") + std::to_string(mt) + name + " is not among the active types of " + when +
         " (ahip_set_active_types, or the type mapping the set was taken from): its forces are invalid; name every model type in use, or return to the automatic set (n = 0)";
}
// Installs `want` (strictly ascending model types; empty: no subset) as the active set: the fused side's model, its prepared weight streams, two-body and LDS tables
// of all three families go (the next evaluation prepares them again for the new set), the byte table full -> compact type and the cutoffs at active x active are uploaded.
static void apply_active(Model &m, const std::vector<int> &want) {
  if (want == m.active) return;
  AHIP_CHECK(hipDeviceSynchronize());        // kernels of an earlier device-resident evaluation may still read the table and the prepared state
  m.active = want;
  m.hm_fused_ready = false;
  m.hm_fused = HostModel();
  free_fused_states(m);
  m.slot_cur = nullptr;
  const int T = m.hm.num_types, A = (int)want.size();
  if (A == 0 || T > FUSED_MAX_TYPES) return;  // (more than 255 types: the shape rule keeps such a model off the fused kernels, nothing reads a table)
  std::vector<unsigned char> tab((size_t)T, (unsigned char)0xFF);
  for (int k = 0; k < A; ++k) tab[(size_t)want[k]] = (unsigned char)k;
  if (!m.slot_dev) AHIP_CHECK(hipMalloc((void **)&m.slot_dev, (size_t)T));
  copy_h2d(m.slot_dev, tab.data(), (size_t)T);
  m.rcut_fused_host.assign((size_t)A * A, 0.0);
  for (int a = 0; a < A; ++a)
    for (int b = 0; b < A; ++b) m.rcut_fused_host[(size_t)a * A + b] = m.rcut_model_host[(size_t)want[a] * T + want[b]];
  if (m.rcut_fused_dev) { AHIP_CHECK(hipFree(m.rcut_fused_dev)); m.rcut_fused_dev = nullptr; }
  AHIP_CHECK(hipMalloc((void **)&m.rcut_fused_dev, (size_t)A * A * sizeof(double)));
  copy_h2d(m.rcut_fused_dev, m.rcut_fused_host.data(), (size_t)A * A * sizeof(double));
}
// The set an evaluation runs with: the explicit one, else -- for a model of more than 16 types only, so that no model the fused kernels already serve changes
// its behaviour -- the types the last type mapping named, else none.
static void resolve_active(Model &m) {
  static const std::vector<int> none;
  apply_active(m, !m.active_set.empty() ? m.active_set : (m.hm.num_types > FUSED_MAX_ACTIVE ? m.active_mapped : none));
}
// the model types a LAMMPS type mapper names (entries outside [0, T) are unmapped LAMMPS types), ascending
static std::vector<int> mapped_types(const Model &m, int ntypes, const int *type_mapper) {
  std::vector<int> v;
  for (int k = 0; k < ntypes; ++k) if (type_mapper[k] >= 0 && type_mapper[k] < m.hm.num_types) v.push_back(type_mapper[k]);
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  return v;
}
// fused_arith=auto falls back to the f32-input MFMA instances for the rest of this model's life (engine.h): the prepared f16x2 weight streams go, the next
// dispatch prepares the f32 ones; said once on stderr and kept for ahip_arith_note
static void arith_degrade(Model &m, const std::string &why) {
  m.arith.degraded = true;
  m.arith.note = "fused_arith=auto: float32 instance (f32-input MFMA) selected: " + why;
  free_fused_states(m);
  std::fprintf(stderr, "[allegro-hip] %s\n", m.arith.note.c_str());
}
// An alarm found at the START of an evaluation, or by an accessor, was raised by an EARLIER device-resident evaluation that nobody waited for: its forces were
// not finite and have been handed out.  That is reported either way; under auto the model also switches to the f32 instance, so the error is reported once.
void fused_poll_alarm(Model &m) {
  if (const int bad = inactive_take(m)) throw ArgError(inactive_message(m, bad, "an EARLIER evaluation"));
  if (!alarm_take(m)) return;
  if (arith_may_degrade(m)) {
    arith_degrade(m, "an earlier evaluation produced a non-finite edge gradient on the f16x2 arithmetic (an activation left float16's range)");
    throw StateError("fused_arith=auto: an EARLIER evaluation produced non-finite forces on the f16x2 arithmetic (an activation left float16's range, or the input was "
                     "not finite); this model now runs on the float32 instance -- re-evaluate from the last valid state");
  }
  throw StateError("fused_arith=f16x2: an edge gradient was not finite (an activation left float16's range, or the input was not finite): the forces of that "
                   "evaluation are invalid; set option fused_arith=f32 (or auto) for this model");
}
}  // namespace ahip

void ahip_model_free(ahip_model *m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  (void)hipDeviceSynchronize();
  if (m->h_alarm) {
    // an alarm of the LAST evaluation of a run is not lost either (void function: said on stderr)
    if (alarm_take(*m)) std::fprintf(stderr, "[allegro-hip] WARNING: the last device-resident evaluation of this model produced non-finite forces on the f16x2 arithmetic "
                                             "(float16 range exceeded); set fused_arith=f32\n");
    (void)hipHostFree(m->h_alarm); m->h_alarm = nullptr;
  }
  free_fused_states(*m);
  neigh_free(*m);
  edges_free(*m);
  m->prim.release();
  free_weights(m->wf);
  free_weights(m->wd);
  if (m->cg_dev) (void)hipFree(m->cg_dev);
  if (m->rcut_model_dev) (void)hipFree(m->rcut_model_dev);
  if (m->rcut_fused_dev) (void)hipFree(m->rcut_fused_dev);
  if (m->slot_dev) (void)hipFree(m->slot_dev);
  for (DevBuf *b : {&m->b_flagwork, &m->b_ilist, &m->b_nloff, &m->b_nlj, &m->b_x, &m->b_ftype, &m->b_mtype, &m->b_f, &m->b_eatom,
                    &m->b_engvir, &m->b_cutsq, &m->b_cnt, &m->b_eoff, &m->b_eii, &m->b_ej, &m->b_rvec, &m->b_ett, &m->b_partial,
                    &m->b_ws, &m->b_misc, &m->b_chk, &m->hv_eoff, &m->hv_eii, &m->hv_ej, &m->hv_rvec, &m->hv_ilist, &m->hv_engvir, &m->b_tile_a0, &m->b_tile_e0, &m->b_centre, &m->b_ntiles, &m->b_vatom,
                    &m->lt_eoff, &m->lt_eii, &m->lt_ej, &m->lt_rvec, &m->lt_ilist, &m->c_x, &m->c_mtype, &m->c_f, &m->c_eatom, &m->c_src, &m->c_shift, &m->c_engvir, &m->c_in, &m->c_xp, &m->c_out, &m->r_xin, &m->r_xhold, &m->r_img, &m->r_disp,
                    &m->q_x[0], &m->q_x[1], &m->q_v[0], &m->q_v[1], &m->q_fixed, &m->q_part, &m->q_fbits, &m->q_state, &m->q_g, &m->q_xc, &m->q_vstate, &m->q_vnow, &m->q_mass, &m->q_mstate,
                    &m->q_thermo, &m->q_frames, &m->q_nstate, &m->q_nthermo, &m->q_fcells})
    b->release();
  for (auto &t : m->slots) for (auto &e : t.ring) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  for (hipEvent_t e : m->f_events) (void)hipEventDestroy(e);
#ifndef AHIP_HOST_EMU
  for (auto &kv : m->pinned) (void)hipHostUnregister(kv.second.first);
#endif
  if (m->counted) g_models_alive.fetch_sub(1);
  delete m;
}

int ahip_model_allow_tf32(const ahip_model *m, int *allow) {
  return guarded([&] {
    if (!m || !allow) throw ArgError("ahip_model_allow_tf32: null argument");
    *allow = m->hm.allow_tf32;
  });
}

int ahip_model_meta(const ahip_model *m, double *r_max, int *num_types, const char **type_names,
                    const double **per_edge_type_cutoff, int *l_max, int *num_tensor_features,
                    int *num_scalar_features, int *num_layers, const char **model_dtype) {
  return guarded([&] {
    require_model(m);
    if (r_max) *r_max = m->hm.r_max;
    if (num_types) *num_types = m->hm.num_types;
    if (type_names) *type_names = m->hm.type_names_joined.c_str();
    if (per_edge_type_cutoff) *per_edge_type_cutoff = m->hm.per_edge_type_cutoff.empty() ? nullptr : m->hm.per_edge_type_cutoff.data();
    if (l_max) *l_max = m->hm.l_max;
    if (num_tensor_features) *num_tensor_features = m->hm.U;
    if (num_scalar_features) *num_scalar_features = m->hm.S;
    if (num_layers) *num_layers = m->hm.num_layers;
    if (model_dtype) *model_dtype = m->hm.model_dtype.c_str();
  });
}

int ahip_set_option(ahip_model *m, const char *key, const char *value) {
  return guarded([&] {
    require_model(m);
    if (!key || !value) throw ArgError("ahip_set_option: NULL key/value");
    const std::string k(key), v(value);
    // an enumerated option: the position of the value among the option's words, which are declared beside its enum in the order of the enumerators
    auto word = [&](const char *words) {
      const int i = word_index(words, v);
      if (i < 0) throw ArgError("option " + k + ": expected " + words);
      return i;
    };
    if (k == "path") {
      m->opt_path = (Model::Path)word(Model::PATH_WORDS);
    } else if (k == "precision") {
      m->opt_precision = (Model::Precision)word(Model::PRECISION_WORDS);
    } else if (k == "fused_arith") {
      const ArithOpt o = (ArithOpt)word(ARITH_OPT_WORDS);
      if (o != m->arith.opt) { m->arith.opt = o; free_fused_states(*m); }
    } else if (k == "fused_tb") {
      const FusedTb o = (FusedTb)word(FUSED_TB_WORDS);
      if (o != m->opt_fused_tb) { m->opt_fused_tb = o; fused_free(*m); }
    } else if (k == "chunk_edges") {
      long long n = std::atoll(value);
      if (n < 1) throw ArgError("option chunk_edges: expected a positive integer");
      m->chunk_edges = n;
    } else if (k == "reserve_wgs") {
      int n = std::atoi(value);
      if (n < 0 || n > 128) throw ArgError("option reserve_wgs: expected 0..128");
      m->reserve_wgs = n;
    } else if (k == "cutoff_compare") {
      m->cutoff_strict = word("le|lt") == 1;
      m->h_cutsq_dev.clear();
    } else if (k == "edge_schedule") {
      m->opt_edge_schedule = (Model::EdgeSchedule)word(Model::EDGE_SCHEDULE_WORDS);
    } else if (k == "tile_pack") {
      m->opt_tile_pack = (Model::TilePack)word(Model::TILE_PACK_WORDS);
    } else if (k == "dense_centres") {
      m->opt_dense_centres = (Model::DenseCentres)word(Model::DENSE_CENTRES_WORDS);
    } else if (k == "wide_tile") {
      const Model::WideTile o = (Model::WideTile)word(Model::WIDE_TILE_WORDS);
      if (o != m->opt_wide_tile) { m->opt_wide_tile = o; fusedlx_free(*m); }      // the per-wave scratch is sized for the shapes the option admits (lx_prepare)
    } else if (k == "lx64_mlp_width") {
      const Model::Lx64MlpWidth o = (Model::Lx64MlpWidth)word(Model::LX64_MLP_WIDTH_WORDS);
      if (o != m->opt_lx64_mlp_width) { m->opt_lx64_mlp_width = o; fusedlx_free(*m); }      // the per-wave scratch follows the row map of the instances the option admits (lx_prepare)
    } else if (k == "env_backward") {
      m->opt_env_backward = (Model::EnvBackward)word(Model::ENV_BACKWARD_WORDS);
    } else if (k == "timing") {
      m->timing = (v == "1" || v == "on" || v == "true");
    } else throw ArgError("unknown option '" + k + "'");
    ++m->list_serial;                        // an option may change what an evaluation runs on: a list held by ahip_compute_cell_reuse is built again
  });
}

namespace ahip {
namespace {
struct Staging {
  std::mutex mu;
  void *p = nullptr;
  // One event pair PER DEVICE: an event belongs to the device that was current when it was created and hipEventRecord refuses a stream of another
  // device; a process that loads models on two devices (ahip_model_load takes the device) copies through the same page-locked buffer with that device's pair.
  std::map<int, std::array<hipEvent_t, 2>> evs;
  hipEvent_t *ev = nullptr;                 // the current device's pair, valid while `mu` is held (set by get())
  static constexpr size_t BYTES = 8u << 20, HALF = BYTES / 2;
  void *get() {
    if (!p) AHIP_CHECK(hipHostMalloc(&p, BYTES, hipHostMallocPortable));
    int dev = 0;
    AHIP_CHECK(hipGetDevice(&dev));
    auto it = evs.find(dev);
    if (it == evs.end()) {
      std::array<hipEvent_t, 2> e{nullptr, nullptr};
      for (int k = 0; k < 2; ++k) AHIP_CHECK(hipEventCreateWithFlags(&e[k], hipEventDisableTiming));
      it = evs.emplace(dev, e).first;
    }
    ev = it->second.data();
    return p;
  }
};
Staging g_staging;      // process-wide, never freed (the runtime may be gone when static destructors run)
}  // namespace

// ---- host-side loops of the host-pointer path, on a few threads ----
// The reference's own host loops are OpenMP loops (pair_nequip_allegro.cpp:371, 488, 566); this library links nothing but libdl, so the three O(nall)
// loops of ahip_compute (type map, position copy into page-locked memory, f +=) and the staging copies run on std::threads instead: AHIP_HOST_THREADS
// (default: min(16, hardware threads)), one thread below 65 536 items.  fn(begin, end) must be safe to run concurrently on disjoint ranges.
int host_threads() {
  static const int n = [] {
    if (const char *e = std::getenv("AHIP_HOST_THREADS")) return std::max(1, std::atoi(e));
    // the CPUs this process may run on, not the machine's: under `mpirun --bind-to core` a rank owns one core, and sixteen workers
    // taking turns on it are slower than one memcpy
    unsigned hw = std::thread::hardware_concurrency();
#ifdef __linux__
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0 && CPU_COUNT(&set) > 0) hw = (unsigned)CPU_COUNT(&set);
#endif
    return (int)std::max(1u, std::min(16u, hw ? hw : 1u));
  }();
  return n;
}
// A persistent pool (created at the first use, never destroyed: worker threads may outlive static destructors): forking and joining eight
// std::threads costs ~0.3 ms, four times per call, which was half of what the loops themselves take at 1 M atoms.
namespace {
struct HostPool {
  std::mutex mu;
  std::condition_variable cv_go, cv_done;
  std::function<void(size_t, size_t)> job;
  size_t n = 0, per = 0;
  unsigned long long gen = 0;
  int pending = 0, nworkers = 0;
  explicit HostPool(int nw) : nworkers(nw) {
    for (int w = 1; w <= nw; ++w) std::thread([this, w] { work(w); }).detach();
  }
  void work(int w) {
    unsigned long long seen = 0;
    for (;;) {
      std::function<void(size_t, size_t)> fn;
      size_t b, e;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv_go.wait(lk, [&] { return gen != seen; });
        seen = gen;
        fn = job;
        b = std::min(n, (size_t)w * per); e = std::min(n, b + per);
      }
      if (b < e) fn(b, e);
      {
        std::lock_guard<std::mutex> lk(mu);
        if (--pending == 0) cv_done.notify_one();
      }
    }
  }
  void run(size_t count, const std::function<void(size_t, size_t)> &fn) {        // one caller at a time (run_mu)
    {
      std::lock_guard<std::mutex> lk(mu);
      job = fn; n = count; per = (count + nworkers) / (nworkers + 1); pending = nworkers; ++gen;
    }
    cv_go.notify_all();
    fn((size_t)0, std::min(count, per));
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [&] { return pending == 0; });
  }
};
std::mutex g_pool_run_mu;
HostPool *g_pool = nullptr;
// a forked child has none of the parent's worker threads: it starts a pool of its own at its first large loop instead of waiting for ever on the parent's
// (the old pool object is leaked on purpose: its mutex may be held by a thread that does not exist in the child)
void pool_atfork_child() { g_pool = nullptr; new (&g_pool_run_mu) std::mutex(); }
const int g_pool_atfork = pthread_atfork(nullptr, nullptr, pool_atfork_child);
}  // namespace
template <class F> static void parallel_for(size_t n, F fn) {
  const int nt = n < 65536 ? 1 : host_threads();
  if (nt <= 1) { fn((size_t)0, n); return; }
  std::lock_guard<std::mutex> lk(g_pool_run_mu);
  if (!g_pool) g_pool = new HostPool(nt - 1);
  g_pool->run(n, std::function<void(size_t, size_t)>(fn));
}
static void parallel_memcpy(void *dst, const void *src, size_t bytes) {
  parallel_for(bytes, [=](size_t b, size_t e) { std::memcpy((char *)dst + b, (const char *)src + b, e - b); });
}

// Pageable host memory <-> device through the page-locked staging buffer, in two halves: the DMA of one half runs while the host copies the other
// (a 184 MB neighbor list used to be 23 memcpy + synchronous-DMA pairs in a row).
void copy_h2d(void *dst_dev, const void *src_host, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_staging.mu);
  char *st = (char *)g_staging.get();
  int k = 0;
  bool used[2] = {false, false};
  for (size_t o = 0; o < bytes; o += Staging::HALF, k ^= 1) {
    const size_t n = std::min(Staging::HALF, bytes - o);
    if (used[k]) AHIP_CHECK(hipEventSynchronize(g_staging.ev[k]));            // the DMA that last read this half
    parallel_memcpy(st + k * Staging::HALF, (const char *)src_host + o, n);
    AHIP_CHECK(hipMemcpyAsync((char *)dst_dev + o, st + k * Staging::HALF, n, hipMemcpyHostToDevice, nullptr));
    AHIP_CHECK(hipEventRecord(g_staging.ev[k], nullptr));
    used[k] = true;
  }
  AHIP_CHECK(hipStreamSynchronize(nullptr));
}
void copy_d2h(void *dst_host, const void *src_dev, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_staging.mu);
  char *st = (char *)g_staging.get();
  // half k holds chunk c: request chunk c + 1 into the other half, then copy chunk c out while that DMA runs
  const size_t nchunk = (bytes + Staging::HALF - 1) / Staging::HALF;
  auto req = [&](size_t c) {
    const size_t o = c * Staging::HALF, n = std::min(Staging::HALF, bytes - o);
    AHIP_CHECK(hipMemcpyAsync(st + (c & 1) * Staging::HALF, (const char *)src_dev + o, n, hipMemcpyDeviceToHost, nullptr));
    AHIP_CHECK(hipEventRecord(g_staging.ev[c & 1], nullptr));
  };
  if (nchunk) req(0);
  for (size_t c = 0; c < nchunk; ++c) {
    AHIP_CHECK(hipEventSynchronize(g_staging.ev[c & 1]));
    if (c + 1 < nchunk) req(c + 1);
    const size_t o = c * Staging::HALF, n = std::min(Staging::HALF, bytes - o);
    parallel_memcpy((char *)dst_host + o, st + (c & 1) * Staging::HALF, n);
  }
}
}  // namespace ahip

// ------------------------------------------------------------------------------------ neighbor list
static void install_list_host(ahip_model *m, int inum, int nall) {
  AHIP_CHECK(hipSetDevice(m->device));
  const size_t nn = m->h_flat_j.size();
  m->b_ilist.reserve(std::max<size_t>(inum, 1) * sizeof(int));
  m->b_nloff.reserve(((size_t)inum + 1) * sizeof(int));
  m->b_nlj.reserve(std::max<size_t>(nn, 1) * sizeof(int));
  copy_h2d(m->b_ilist.p, m->h_ilist.data(), (size_t)inum * sizeof(int));
  copy_h2d(m->b_nloff.p, m->h_off32.data(), ((size_t)inum + 1) * sizeof(int));
  copy_h2d(m->b_nlj.p, m->h_flat_j.data(), nn * sizeof(int));
  m->d_ilist = m->b_ilist.as<int>();
  m->d_nloff = m->b_nloff.as<int>();
  m->d_nlj = m->b_nlj.as<int>();
  m->inum = inum; m->nall = nall; m->nneigh = (long long)nn; m->have_list = true;
  ++m->list_serial;
  m->max_list_row = 0;
  for (int ii = 0; ii < inum; ++ii) m->max_list_row = std::max(m->max_list_row, m->h_off32[ii + 1] - m->h_off32[ii]);
}

static void check_list_dims(int inum, int nall) {
  if (inum < 0 || nall < inum) throw ArgError("neighbor list: need 0 <= inum <= nall");
}

int ahip_neigh_update(ahip_model *m, int inum, int nall, const int *ilist, const int *numneigh,
                      const int *const *firstneigh, int neighmask) {
  return guarded([&] {
    require_model(m);
    check_list_dims(inum, nall);
    if (inum > 0 && (!ilist || !numneigh || !firstneigh)) throw ArgError("ahip_neigh_update: NULL list pointer");
    m->h_ilist.assign(ilist, ilist + inum);
    m->h_off32.resize((size_t)inum + 1);
    long long tot = 0;
    for (int ii = 0; ii < inum; ++ii) {
      int i = ilist[ii];
      if (i < 0 || i >= nall) throw ArgError("neighbor list: ilist entry out of range");
      m->h_off32[ii] = (int)tot;
      tot += numneigh[i];
      if (tot > 2147483000LL) throw UnsupportedError("neighbor list too large for 32-bit offsets; use more ranks");
    }
    m->h_off32[inum] = (int)tot;
    m->h_flat_j.resize((size_t)tot);
    for (int ii = 0; ii < inum; ++ii) {
      int i = ilist[ii];
      const int *jl = firstneigh[i];
      int *dst = m->h_flat_j.data() + m->h_off32[ii];
      for (int jj = 0; jj < numneigh[i]; ++jj) {
        int j = jl[jj] & neighmask;                          // pair_nequip_allegro.cpp:496
        if (j < 0 || j >= nall) throw ArgError("neighbor list: neighbour index out of range");
        dst[jj] = j;
      }
    }
    install_list_host(m, inum, nall);
  });
}

int ahip_neigh_update_csr(ahip_model *m, int inum, int nall, const int *ilist, const long long *offsets,
                          const int *neigh, int neighmask) {
  return guarded([&] {
    require_model(m);
    check_list_dims(inum, nall);
    if (inum > 0 && (!ilist || !offsets)) throw ArgError("ahip_neigh_update_csr: NULL list pointer");
    m->h_ilist.assign(ilist, ilist + inum);
    m->h_off32.resize((size_t)inum + 1);
    long long tot = inum > 0 ? offsets[inum] : 0;
    if (tot > 2147483000LL) throw UnsupportedError("neighbor list too large for 32-bit offsets; use more ranks");
    if (tot > 0 && !neigh) throw ArgError("ahip_neigh_update_csr: NULL neigh");
    for (int ii = 0; ii <= inum; ++ii) {
      long long o = inum > 0 ? offsets[ii] : 0;
      if (o < 0 || o > tot || (ii > 0 && o < offsets[ii - 1])) throw ArgError("neighbor list: offsets not monotone");
      m->h_off32[ii] = (int)o;
    }
    for (int ii = 0; ii < inum; ++ii)
      if (ilist[ii] < 0 || ilist[ii] >= nall) throw ArgError("neighbor list: ilist entry out of range");
    m->h_flat_j.resize((size_t)tot);
    for (long long p = 0; p < tot; ++p) {
      int j = neigh[p] & neighmask;
      if (j < 0 || j >= nall) throw ArgError("neighbor list: neighbour index out of range");
      m->h_flat_j[(size_t)p] = j;
    }
    install_list_host(m, inum, nall);
  });
}

int ahip_neigh_update_dev(ahip_model *m, int inum, int nall, const int *ilist_dev, const int *offsets_dev,
                          const int *neigh_dev, long long nneigh_total) {
  return guarded([&] {
    require_model(m);
    check_list_dims(inum, nall);
    if (inum > 0 && (!ilist_dev || !offsets_dev)) throw ArgError("ahip_neigh_update_dev: NULL list pointer");
    m->d_ilist = ilist_dev; m->d_nloff = offsets_dev; m->d_nlj = neigh_dev;
    m->inum = inum; m->nall = nall; m->nneigh = nneigh_total; m->have_list = true;
    ++m->list_serial;
    // longest row: bounds the degree of every centre until the next hand-over, which is what lets the per-step calls run without a read-back
    AHIP_CHECK(hipSetDevice(m->device));
    m->max_list_row = edges_max_row(*m, inum, offsets_dev);
  });
}

// ------------------------------------------------------------------------------------ compute
namespace ahip {
void timing_drain(Model &m, TimingSlot &t, size_t keep) {
  (void)m;
  while (t.head - t.tail > keep) {
    const auto &e = t.ring[t.tail % TIMING_RING];
    float ms = 0;
    if (hipEventSynchronize(e.second) == hipSuccess && hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) { t.sum_ms += ms; ++t.count; }
    else (void)hipGetLastError();
    ++t.tail;
  }
}
}  // namespace ahip
// everything recorded since the last report -> timing_names / timing_ms (sums) / timing_counts; waits for the recorded stages
static void collect_timings(ahip_model *m) {
  m->timing_names.clear();
  m->timing_ms.clear();
  m->timing_counts.clear();
  if (!m->timing) return;
  for (auto &t : m->slots) {
    timing_drain(*m, t, 0);
    if (t.count == 0) continue;
    if (!m->timing_names.empty()) m->timing_names += ";";
    m->timing_names += t.name;
    m->timing_ms.push_back(t.sum_ms);
    m->timing_counts.push_back((double)t.count);
    t.sum_ms = 0; t.count = 0;
  }
}

// The kernels keep an edge iff rsq <= bound.  bound = cut^2 gives the host path's `<=` (pair_nequip_allegro.cpp:507); the largest
// double below cut^2 gives the KOKKOS path's strict `<` (pair_nequip_allegro_kokkos.cpp:174) without touching the kernels.
static double cutsq_bound(const ahip_model *m, double c) {
  const double c2 = c * c;
  return m->cutoff_strict ? std::nextafter(c2, 0.0) : c2;
}

static __global__ void k_add_n(long long n, double *dst, const double *src) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) dst[t] += src[t];
}
static __global__ void k_copy_centres(int inum, const int *ilist, double *dst, const double *src) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < inum) dst[ilist[t]] = src[ilist[t]];
}
static __global__ void k_add7(double *dst, const double *src) { if (threadIdx.x < 7) dst[threadIdx.x] += src[threadIdx.x]; }

// The few centres that do not fit a tile of the wide fused kernel: layer-at-a-time float32 kernels on a compact copy of their
// edges; forces and per-atom energies accumulate into the same arrays, energy / virial partial sums are added.
static void heavy_generic(ahip_model *m, const ComputeArgs &a) {
  edges_compact_heavy(*m, a);
  m->hv_engvir.reserve(8 * sizeof(double));
  auto swap_in = [&]() {
    std::swap(m->b_eoff, m->hv_eoff); std::swap(m->b_eii, m->hv_eii); std::swap(m->b_ej, m->hv_ej); std::swap(m->b_rvec, m->hv_rvec);
  };
  const int *il = m->d_ilist;
  const int inum = m->inum;
  const long long ne = m->nedges;
  swap_in();
  m->d_ilist = m->hv_ilist.as<int>();
  m->inum = m->nheavy; m->nedges = m->hv_nedges;
  ComputeArgs a2 = a;
  a2.engvir = m->hv_engvir.as<double>();
  try { generic_run<float>(*m, a2); }
  catch (...) { swap_in(); m->d_ilist = il; m->inum = inum; m->nedges = ne; throw; }
  swap_in(); m->d_ilist = il; m->inum = inum; m->nedges = ne;
  hipLaunchKernelGGL(k_add7, dim3(1), dim3(64), 0, a.stream, a.engvir, a2.engvir);
}

// The fused kernel family that serves the model (fused_shapes.h): k_fused (l_max = 1, up to 32 tensor features), k_fused_lx (l_max = 2, up to 32), k_fused_lx2
// (up to 64, l_max = 2 or an l_max = 1 model lifted), or none (why: the reasons of both gates).  Not cached: it depends on arith.force_f32 / arith.degraded
// (MLP depth 1 / 3 and read-out depth 2 need f16x2), which the self-check and an ArithDegraded fallback change.
static FusedFamily fused_family(const Model &m, std::string *why) {
  std::string why1, why2;
  if (fused_model_supported(m, &why1)) return FusedFamily::k_fused;
  if (fusedlx_model_supported(m, &why2)) return fused_shape_class(m.hm);
  if (why) *why = why1 + "; " + why2;
  return FusedFamily::none;
}

static bool fused_run_family(ahip_model *m, FusedFamily fam, const ComputeArgs &a, std::string *why) {
  if (fam == FusedFamily::k_fused) return fused_run(*m, a, why);
  if (fam == FusedFamily::lx32) return fusedlx_run(*m, a, why);
  if (fam == FusedFamily::lx64) return fusedlx2_run(*m, a, why);
  return false;
}
// Option dense_centres=split behind the two-pass edge build, which has listed m->nheavy > 0 heavy centres: the fused kernel runs on the compact copy of the list
// WITHOUT them (edges.hip: edges_compact_light), swapped in for the duration of its run.  To the kernel's host driver that copy is an ordinary two-pass list with its
// counts on the host: its largest degree is the largest LIGHT degree, so k_fused picks the 4- or 8-wave tile shape from that, the stand-alone packing kernels give
// every slot to a light centre, and no kernel's device code knows about heavy centres.  Everything is restored before heavy_generic evaluates the listed centres.
static bool fused_run_light(ahip_model *m, FusedFamily fam, const ComputeArgs &a, std::string *why) {
#ifndef AHIP_HOST_EMU                        // (the host-emulation build has no fused kernel and never gets here)
  edges_compact_light(*m, a);
#endif
  auto swap_in = [&]() {
    std::swap(m->b_eoff, m->lt_eoff); std::swap(m->b_eii, m->lt_eii); std::swap(m->b_ej, m->lt_ej); std::swap(m->b_rvec, m->lt_rvec);
  };
  const int *il = m->d_ilist;
  const int inum = m->inum, nheavy = m->nheavy, thresh = m->heavy_thresh, maxdeg = m->last_max_deg;
  const long long ne = m->nedges;
  auto restore = [&]() {
    swap_in();
    m->d_ilist = il; m->inum = inum; m->nedges = ne; m->nheavy = nheavy; m->heavy_thresh = thresh; m->last_max_deg = maxdeg;
    m->have_ett = false;                     // the packed edge types written for the fused kernel belong to the copy
  };
  swap_in();
  m->d_ilist = m->lt_ilist.as<int>();
  m->inum = inum - nheavy; m->nedges = ne - m->heavy_listed_edges; m->nheavy = 0; m->heavy_thresh = 0; m->last_max_deg = m->light_max_deg;
  bool ok = false;
  try { ok = fused_run_family(m, fam, a, why); }
  catch (...) { restore(); throw; }
  m->last_tile_edges = m->nedges;
  restore();
  return ok;
}

static void run_model_once(ahip_model *m, const ComputeArgs &a);
// dispatch with the auto fallback: a prepare step that finds the model outside the f16x2 split's reach (ArithDegraded) costs one more dispatch, on f32
static void run_model_dispatch(ahip_model *m, const ComputeArgs &a) {
  try { run_model_once(m, a); }
  catch (const ArithDegraded &d) {
    arith_degrade(*m, d.why);
    run_model_once(m, a);
  }
}
static __global__ void k_chk_reduce(long long n, const double *a, const double *b, unsigned long long *out) {
  // out[0] = max |a - b|, out[1] = max |a| as bit patterns (non-negative doubles order like their bits); a non-finite difference maps to +inf
  double d = 0.0, f = 0.0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    double di = fabs(a[i] - b[i]);
    if (!(di < 1.0e300)) di = 1.0e300;
    d = fmax(d, di); f = fmax(f, fabs(a[i]));
  }
  atomicMax(out, __builtin_bit_cast(unsigned long long, d));          // one pair of atomics per thread of a 1024 x 256 grid, once per model: no wave reduction needed
  atomicMax(out + 1, __builtin_bit_cast(unsigned long long, f));
}
// First evaluation of a model whose fused_arith=auto resolves to f16x2 (VERDICT r05 #3c): the same centres once on the f32 instance, once on f16x2, forces
// compared; f16x2 stays only if max|dF| <= 1e-5 max|F| (float32-equivalence on THIS model and THIS configuration, not on the builder's samples) and no
// alarm was raised.  Cost: two extra evaluations and two weight-stream builds, once per model (per pair_coeff).  Energies / virial / per-atom energies are the
// second pass's (or the fallback's); f gets the chosen pass added, as always.
static void run_model_selfcheck(ahip_model *m, const ComputeArgs &a) {
  m->arith.checked = true;
  const long long nf = 3LL * (a.nlocal + a.nghost);
  m->b_chk.reserve((size_t)(2 * nf + 16) * sizeof(double));
  double *f32f = m->b_chk.as<double>(), *f16f = f32f + nf, *ev = f16f + nf;
  unsigned long long *red = (unsigned long long *)(ev + 8);
  hipStream_t s = a.stream;
  auto add_to_f = [&]() { if (nf > 0) hipLaunchKernelGGL(k_add_n, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s, nf, a.f, f16f); };      // the kept pass's forces into the caller's
  AHIP_CHECK(hipMemsetAsync(m->b_chk.p, 0, (size_t)(2 * nf + 16) * sizeof(double), s));
  ComputeArgs a1 = a;
  a1.f = f32f; a1.eatom = nullptr; a1.engvir = ev;
  m->arith.force_f32 = true;
  free_fused_states(*m);
  try { run_model_dispatch(m, a1); } catch (...) { m->arith.force_f32 = false; free_fused_states(*m); throw; }
  m->arith.force_f32 = false;                     // (a shape without a float32 fused instance -- MLP depth 1 / 3 -- was just evaluated by the layer-at-a-time float32 kernels)
  free_fused_states(*m);
  ComputeArgs a2 = a;
  a2.f = f16f;
  run_model_dispatch(m, a2);                 // (a prepare-time fallback inside lands on f32 as well: the comparison below is then trivially green)
  if (m->last_path != fused_path_name(AR_F16X2) && !m->arith.degraded) {
    // this LIST went down the layer-at-a-time path (a centre with more edges than a tile holds): nothing was checked; a later list gets its chance, three times at most
    if (++m->arith.check_attempts < 3) m->arith.checked = false;
    add_to_f();
    return;
  }
  hipLaunchKernelGGL(k_chk_reduce, dim3(1024), dim3(256), 0, s, nf, f32f, f16f, red);
  unsigned long long hred[2] = {0, 0};
  AHIP_CHECK(hipMemcpyAsync(hred, red, sizeof(hred), hipMemcpyDeviceToHost, s));
  AHIP_CHECK(hipStreamSynchronize(s));
  double dmax, fmax_;
  std::memcpy(&dmax, &hred[0], 8); std::memcpy(&fmax_, &hred[1], 8);
  const bool alarm = alarm_take(*m);
  const bool ok = !alarm && dmax <= 1.0e-5 * fmax_ + 1.0e-30;
  char buf[256];
  if (m->arith.degraded) {                   // fell back while preparing: f16f holds the float32 result
    add_to_f();
    return;
  }
  if (ok) {
    std::snprintf(buf, sizeof(buf), "fused_arith=auto: f16x2 kept: first evaluation within %.2e max|F| of the float32 instance (max|dF| %.3e, max|F| %.3e; bar 1e-5)",
                  fmax_ > 0 ? dmax / fmax_ : 0.0, dmax, fmax_);
    m->arith.note = buf;
    add_to_f();
    return;
  }
  std::snprintf(buf, sizeof(buf), "first-evaluation self-check: f16x2 %s (max|dF| %.3e vs the float32 instance, max|F| %.3e; bar 1e-5 max|F|)",
                alarm ? "raised the float16-range alarm" : "disagrees with the float32 instance", dmax, fmax_);
  arith_degrade(*m, buf);
  run_model_dispatch(m, a);                  // float32, straight into the caller's arrays
}
static void run_model(ahip_model *m, const ComputeArgs &a) {
  fused_poll_alarm(*m);                      // raised by an EARLIER device-resident evaluation (nobody waits for those kernels)
  resolve_active(*m);                        // the active types of this evaluation (a change drops the prepared fused state)
  const bool wants_check = !m->arith.checked && arith_may_degrade(*m) && m->inum > 0 && !model_runs_f64(*m) && m->opt_path != Model::Path::Generic &&
                           !m->hm.allow_tf32 && fused_family(*m, nullptr) != FusedFamily::none &&
                           std::getenv("AHIP_NO_ARITH_SELFCHECK") == nullptr;
  if (wants_check) {
    run_model_selfcheck(m, a);
    if (m->arith.checked) m->b_chk.release();      // two force arrays of the whole system: not kept for the model's life (hipFree waits for the kernels that still read them)
  } else run_model_dispatch(m, a);
}
static void run_model_once(ahip_model *m, const ComputeArgs &a) {
  m->nedges = 0;
  m->slot_cur = nullptr;
  m->last_heavy_centres = 0; m->last_heavy_edges = 0; m->last_tile_edges = -1;
  // W restarts with every dispatch: it always belongs to the evaluation whose forces reach f (self-check passes, ArithDegraded re-dispatch, float32 fallback)
  if (a.vatom) AHIP_CHECK(hipMemsetAsync(a.vatom, 0, (size_t)(a.nlocal + a.nghost) * 9 * sizeof(double), a.stream));
  const bool f64 = model_runs_f64(*m);
  // the 7 energy / virial sums start from zero: the single-pass edge build clears them in its first kernel, every other way here
  if (m->inum == 0 || f64) AHIP_CHECK(hipMemsetAsync(a.engvir, 0, 7 * sizeof(double), a.stream));
  if (m->inum == 0) return;                                   // empty sub-domain (pair_nequip_allegro.cpp:340-341)
  if (f64) {
    if (m->opt_path == Model::Path::Fused) throw UnsupportedError("the fused MFMA path computes in float32; use path=generic for float64");
    build_edges<double>(*m, a);
    generic_run<double>(*m, a);
    m->last_path = "generic_f64";
    return;
  }
  std::string why;
  const FusedFamily fam = m->opt_path == Model::Path::Generic ? FusedFamily::none : fused_family(*m, &why);
  const bool wide = fam == FusedFamily::lx32 || fam == FusedFamily::lx64;
  // a fused kernel will run on the model restricted to its active types: the writers of fused-side types translate through the byte table (everything else, the
  // heavy centres of the layer-at-a-time kernels included, keeps full model types)
  if (fam != FusedFamily::none && !m->active.empty()) m->slot_cur = m->slot_dev;
  m->have_ett = false;
  m->nheavy = 0;
  // the largest tile of the wide kernel that will run: 64 slots, or 128 under wide_tile=auto where k_fused_lx has its 8-wave shape for this model
  const int lx_slots = wide ? lx_max_tile_slots(*m, fam) : 0;
  m->heavy_thresh = lx_slots;
  // Tile packing rides on the edge build when the tile shape is known before it runs: k_fused with every list row <= 64 entries (4-wave tiles:
  // 64 slots, 6 centres), the wide kernels always (64 slots, 4 centres) unless the 128-slot shape of k_fused_lx may be needed (wide_tile=auto and list rows above 64).  Otherwise (shape chosen on the device, two-pass edge build) the
  // stand-alone packing kernels run after it, as before.
  m->pack_slots = m->pack_maxa = 0;
  // ... and up to 262 144 centres per call: the packing runs on the scanning wave of every unit, i.e. serially inside the edge build, and costs there what
  // the stand-alone kernels cost beside it once they have a chip to spread over (1 M atoms: 0.062 vs 0.064 ms); below that the six launches they need are
  // the cost (10 648 atoms: 0.026 ms, 125 000: 0.056 ms, three times per step in the overlapped multi-rank schedule)
  if (m->opt_tile_pack != Model::TilePack::Separate && (m->inum <= 262144 || m->opt_tile_pack == Model::TilePack::Fused)) {
    if (fam == FusedFamily::k_fused) { if (m->max_list_row >= 0 && m->max_list_row <= FUSED_TILE_SLOTS) { m->pack_slots = FUSED_TILE_SLOTS; m->pack_maxa = FUSED_TILE_MAXA; } }
    else if (wide && (lx_slots == LX_TILE_SLOTS || (m->max_list_row >= 0 && m->max_list_row <= LX_TILE_SLOTS))) { m->pack_slots = LX_TILE_SLOTS; m->pack_maxa = LX_TILE_MAXA; }
  }
  m->tiles_packed = false;
  const bool two_pass = !edges_build_f32(*m, a);
  if (two_pass) {
    m->nheavy = 0; m->heavy_thresh = 0;
    AHIP_CHECK(hipMemsetAsync(a.engvir, 0, 7 * sizeof(double), a.stream));
    // option dense_centres=split: the two-pass build lists the heavy centres of the fused family that will run as well (k_fused: more edges than its 8-wave tile
    // holds; the wide kernels: as on the single-pass route) and leaves heavy_thresh, nheavy and the largest light degree on the host with its own counts
    const bool split = m->opt_dense_centres == Model::DenseCentres::Split && fam != FusedFamily::none;
    build_edges<float>(*m, a, split ? (wide ? lx_slots : FUSED_MAX_TILE_SLOTS) : 0);
  }
#ifdef AHIP_EXPERIMENT_SWITCHES      // never in the product build: a switch that skips the model returns no forces
  static const bool edges_only = std::getenv("AHIP_EDGES_ONLY") != nullptr;     // timing experiments on the edge build alone
  if (edges_only) { m->last_path = "edges_only"; return; }
#endif
  bool fused_ok = false;
  if (m->opt_path != Model::Path::Generic) {
    m->arith.last = AR_F32;
    // heavy centres listed by the two-pass build (dense_centres=split; the single-pass build leaves its counts in flight): the give-up rule of the wide kernels
    // (fused_lx_common.h: lx_list_fits) for every family, else the fused kernel on the list without them
    const bool light = two_pass && m->nheavy > 0;
    if (light && (long long)m->nheavy * 8 > m->inum)
      why = std::to_string(m->nheavy) + " of " + std::to_string(m->inum) + " centres have more than " + std::to_string(m->heavy_thresh) +
            " edges (dense_centres=split hands over at most one centre in eight)";
    else if (light) fused_ok = fused_run_light(m, fam, a, &why);
    else fused_ok = fused_run_family(m, fam, a, &why);
    if (!fused_ok && m->opt_path == Model::Path::Fused) throw UnsupportedError("fused path unavailable: " + why);
  }
  if (fused_ok) {
    // wide kernels: the number of centres left to the layer-at-a-time kernels is read now, with the model kernel already enqueued
    // (the copy sits in front of it in the stream, so the host waits for the edge build only); k_fused never asks (heavy_thresh = 0, or the two-pass build's counts, which are on the host)
    if (m->heavy_thresh > 0) edges_counts(*m);
    if (m->nheavy > 0) {
      heavy_generic(m, a);
      m->last_heavy_centres = m->nheavy; m->last_heavy_edges = m->hv_nedges;
    }
    // "fused_tf32eq": the two-term bf16 split the model file licensed with allow_tf32 = 1 (fused.hip); everything else is float32-exact
    // "fused_f16x2" / "fused_bf16x3": float32-equivalent splits on the f16 / bf16 matrix cores (fused_h.h, fused.hip); "fused_f32": exact fmaf chains
    m->last_path = fused_path_name(m->arith.last);
    return;
  }
  edges_counts(*m);
  generic_run<float>(*m, a);
  m->last_path = "generic_f32";
}

// `compute allegro` names this model returns; "atomic_virial" [nall][9] is this library's own (no nequip key): the per-atom virial
// W_j[a][b] = -sum over the edges e = (i -> j) of r_e[a] dE/dr_e[b], each edge owned by its NEIGHBOUR j (ghost rows reverse-communicated by the caller)
static void check_output_names(const ahip_model *m) {
  for (const std::string &nm : m->custom_names)
    if (nm != "atomic_energy" && nm != "forces" && nm != "virial" && nm != "total_energy" && nm != "atomic_virial")
      throw ArgError("model output '" + nm + "' not found (this model returns atomic_energy, forces, virial, total_energy, atomic_virial)");
}
static bool want_atomic_virial(const ahip_model *m) {
  return std::find(m->custom_names.begin(), m->custom_names.end(), "atomic_virial") != m->custom_names.end();
}
static double *vatom_buffer(ahip_model *m, int nall) {
  m->b_vatom.reserve((size_t)std::max(nall, 1) * 9 * sizeof(double));
  return m->b_vatom.as<double>();
}
// The `compute allegro` output table, i.e. the model's output dict entries (pair_nequip_allegro.cpp:403-406), rows for locals AND ghosts: from h_f,
// h_eatom, h_mtype (host copies of this evaluation), b_vatom and ev[7] (energy, virial xx yy zz xy xz yz), after the stream has been synchronised.
// ilist: the host centre list of the inum centres, or null for centres 0 .. inum - 1.
static void store_custom_outputs(ahip_model *m, int nall, int inum, const int *ilist, const double *ev) {
  std::vector<double> ae(nall);
  const HostTensor &shift = m->hm.get("shift");
  for (int i = 0; i < nall; ++i) ae[i] = shift.data[m->h_mtype[i]];        // ghosts: no centre edges -> shift only
  for (int ii = 0; ii < inum; ++ii) { const int i = ilist ? ilist[ii] : ii; ae[i] = m->h_eatom[i]; }
  double tot = 0;
  for (double v : ae) tot += v;
  for (const std::string &nm : m->custom_names) {
    if (nm == "atomic_energy") m->custom_out[nm] = ae;
    else if (nm == "forces") m->custom_out[nm] = m->h_f;
    else if (nm == "total_energy") m->custom_out[nm] = {tot};
    else if (nm == "atomic_virial") {
      std::vector<double> &w = m->custom_out[nm];
      w.resize((size_t)nall * 9);
      if (nall > 0) copy_d2h(w.data(), m->b_vatom.p, w.size() * sizeof(double));
    } else m->custom_out[nm] = {ev[1], ev[4], ev[5], ev[4], ev[2], ev[6], ev[5], ev[6], ev[3]};    // [3][3] from xx yy zz xy xz yz
  }
}

// Page-locks a persistent host vector for as long as it keeps its storage: copies from / into pageable memory are staged by the runtime
// and "asynchronous" in name only; the vectors of the host-pointer path only ever grow, so this registers once per growth.
// resize_pinned: a growing resize frees the old storage, so the registration of that storage is dropped FIRST (unregistering a freed
// range afterwards, or a new allocation landing on the still-registered old range, was possible at re-neighborings that grow nall)
template <class T> static void unpin_if_growing(ahip::Model *m, std::vector<T> &v, size_t n) {
#ifndef AHIP_HOST_EMU
  if (n <= v.capacity()) return;
  auto it = m->pinned.find((const void *)&v);
  if (it != m->pinned.end()) { (void)hipHostUnregister(it->second.first); m->pinned.erase(it); }
#endif
}
template <class T> static void pin_host(ahip::Model *m, std::vector<T> &v) {
#ifndef AHIP_HOST_EMU
  void *p = (void *)v.data();
  const size_t bytes = v.capacity() * sizeof(T);
  auto it = m->pinned.find((const void *)&v);
  if (it != m->pinned.end() && it->second.first == p && it->second.second == bytes) return;
  if (it != m->pinned.end()) { (void)hipHostUnregister(it->second.first); m->pinned.erase(it); }
  if (p && bytes && hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess) m->pinned[(const void *)&v] = {p, bytes};
  else (void)hipGetLastError();          // registration is an optimisation: pageable copies still work
#endif
}

int ahip_compute(ahip_model *m, int nlocal, int nghost, const double *x, const int *type, int ntypes,
                 const int *type_mapper, const double *cutoff_matrix, double *f, double *eatom, double *eng,
                 double *virial) {
  return guarded([&] {
    require_model(m);
    if (!m->have_list) throw StateError("ahip_compute called before ahip_neigh_update");
    if (nlocal < 0 || nghost < 0) throw ArgError("ahip_compute: negative atom count");
    const int nall = nlocal + nghost;
    if (nall != m->nall) throw StateError("ahip_compute: nlocal+nghost differs from the neighbor list's nall; call ahip_neigh_update after re-neighboring");
    if (nall > 0 && (!x || !type || !f)) throw ArgError("ahip_compute: NULL x/type/f");
    if (ntypes <= 0 || !type_mapper || !cutoff_matrix) throw ArgError("ahip_compute: bad ntypes/type_mapper/cutoff_matrix");
    if (!eng) throw ArgError("ahip_compute: eng is NULL");
    AHIP_CHECK(hipSetDevice(m->device));
    hipStream_t s = nullptr;
    *eng = 0;
    if (virial) for (int k = 0; k < 6; ++k) virial[k] = 0;
    m->custom_out.clear();
    if (m->inum == 0) return;          // empty domain: nothing is stored (compute_allegro.cpp:106-112)
    check_output_names(m);                                             // the reference's output.at(name) (:404-405)
    const bool want_eatom = eatom != nullptr || !m->custom_names.empty();
    double *vatom = want_atomic_virial(m) ? vatom_buffer(m, nall) : nullptr;

    // types: LAMMPS 1-based -> filter index (type-1) and model type (pair_nequip_allegro.cpp:576)
    unpin_if_growing(m, m->h_ftype, (size_t)nall); unpin_if_growing(m, m->h_mtype, (size_t)nall);
    m->h_ftype.resize(nall); m->h_mtype.resize(nall);
    {
      std::atomic<int> bad_range{0}, bad_map{0};           // first offending LAMMPS type of each kind (0: none): the threads report, this thread throws
      const int nmt = m->hm.num_types;
      int *const hft = m->h_ftype.data(), *const hmt = m->h_mtype.data();
      parallel_for((size_t)nall, [&, hft, hmt](size_t b, size_t e) {
        for (size_t i = b; i < e; ++i) {
          const int t = type[i];
          if (t < 1 || t > ntypes) { bad_range.store(t ? t : -1); hft[i] = 0; hmt[i] = 0; continue; }
          const int mt = type_mapper[t - 1];
          if (mt < 0 || mt >= nmt) { bad_map.store(t); hft[i] = 0; hmt[i] = 0; continue; }
          hft[i] = t - 1; hmt[i] = mt;
        }
      });
      if (bad_range.load()) throw ArgError("ahip_compute: atom type out of range");
      if (bad_map.load()) throw ArgError("ahip_compute: LAMMPS type " + std::to_string(bad_map.load()) + " is not mapped to a model type (all pair coeffs are not set)");
    }
    m->active_mapped = mapped_types(*m, ntypes, type_mapper);
    std::vector<double> cutsq((size_t)ntypes * ntypes);
    for (size_t k = 0; k < cutsq.size(); ++k) cutsq[k] = cutsq_bound(m, cutoff_matrix[k]);
    m->b_x.reserve((size_t)nall * 3 * sizeof(double));
    m->b_ftype.reserve((size_t)nall * sizeof(int));
    m->b_mtype.reserve((size_t)nall * sizeof(int));
    m->b_f.reserve((size_t)nall * 3 * sizeof(double));
    m->b_eatom.reserve((size_t)nall * sizeof(double));
    m->b_engvir.reserve(8 * sizeof(double));
    m->b_cutsq.reserve(cutsq.size() * sizeof(double));
    // positions: one host copy into a page-locked buffer, then a true DMA (LAMMPS' atom->x itself is pageable and not ours to register)
    unpin_if_growing(m, m->h_x, (size_t)nall * 3);
    m->h_x.resize((size_t)nall * 3);
    pin_host(m, m->h_x); pin_host(m, m->h_ftype); pin_host(m, m->h_mtype);
    {
      // in chunks: the DMA of chunk c runs while the threads copy chunk c + 1 into the page-locked buffer
      const size_t tot = (size_t)nall * 3 * sizeof(double), CH = 16u << 20;
      for (size_t o = 0; o < tot; o += CH) {
        const size_t n = std::min(CH, tot - o);
        parallel_memcpy((char *)m->h_x.data() + o, (const char *)x + o, n);
        AHIP_CHECK(hipMemcpyAsync((char *)m->b_x.p + o, (const char *)m->h_x.data() + o, n, hipMemcpyHostToDevice, s));
      }
    }
    AHIP_CHECK(hipMemcpyAsync(m->b_ftype.p, m->h_ftype.data(), (size_t)nall * sizeof(int), hipMemcpyHostToDevice, s));
    AHIP_CHECK(hipMemcpyAsync(m->b_mtype.p, m->h_mtype.data(), (size_t)nall * sizeof(int), hipMemcpyHostToDevice, s));
    AHIP_CHECK(hipMemcpyAsync(m->b_cutsq.p, cutsq.data(), cutsq.size() * sizeof(double), hipMemcpyHostToDevice, s));
    m->h_cutsq_dev.clear();
    unpin_if_growing(m, m->h_f, (size_t)nall * 3);
    m->h_f.resize((size_t)nall * 3);
    pin_host(m, m->h_f);
    double ev[7];
    constexpr size_t FCH = 8u << 20;
    const size_t ftot = (size_t)nall * 3 * sizeof(double), nfch = (ftot + FCH - 1) / FCH;
    while (m->f_events.size() < nfch + 1) { hipEvent_t e; AHIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); m->f_events.push_back(e); }
    // (twice at most: an evaluation whose f16x2 kernels raise the float16-range alarm under fused_arith=auto is repeated on the float32 instance)
    for (int attempt = 0;; ++attempt) {
    AHIP_CHECK(hipMemsetAsync(m->b_f.p, 0, (size_t)nall * 3 * sizeof(double), s));
    if (want_eatom) AHIP_CHECK(hipMemsetAsync(m->b_eatom.p, 0, (size_t)nall * sizeof(double), s));

    ComputeArgs a{nlocal, nghost, m->b_x.as<double>(), m->b_ftype.as<int>(), m->b_cutsq.as<double>(), ntypes,
                  m->b_mtype.as<int>(), m->b_f.as<double>(), want_eatom ? m->b_eatom.as<double>() : nullptr,
                  m->b_engvir.as<double>(), s, vatom};
    run_model(m, a);

    // Order on the stream: the 7 energy / virial sums and an event (the kernel has finished once it fires: the float16-range alarm of THIS evaluation is
    // valid and is reported by this call, before f is touched), then the forces in chunks, each behind an event: the host adds chunk c into f while
    // the DMA of chunk c + 1 runs; the per-atom energies last.
    AHIP_CHECK(hipMemcpyAsync(ev, m->b_engvir.p, 7 * sizeof(double), hipMemcpyDeviceToHost, s));
    AHIP_CHECK(hipEventRecord(m->f_events[nfch], s));
    for (size_t c = 0; c < nfch; ++c) {
      const size_t o = c * FCH, n = std::min(FCH, ftot - o);
      AHIP_CHECK(hipMemcpyAsync((char *)m->h_f.data() + o, (const char *)m->b_f.p + o, n, hipMemcpyDeviceToHost, s));
      AHIP_CHECK(hipEventRecord(m->f_events[c], s));
    }
    if (want_eatom) {
      unpin_if_growing(m, m->h_eatom, (size_t)nall);
      m->h_eatom.resize(nall);
      pin_host(m, m->h_eatom);
      AHIP_CHECK(hipMemcpyAsync(m->h_eatom.data(), m->b_eatom.p, (size_t)nall * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    AHIP_CHECK(hipEventSynchronize(m->f_events[nfch]));
    if (const int bad = inactive_take(*m)) {   // an explicit active set that leaves out a type in use: reported by this call, before f is touched
      (void)hipStreamSynchronize(s);
      throw ArgError("ahip_compute: " + inactive_message(*m, bad, "this evaluation") + " (nothing was added to f)");
    }
    if (alarm_take(*m)) {                    // raised by THIS evaluation: nothing of it has touched the caller's arrays yet
      (void)hipStreamSynchronize(s);         // (the copies into the page-locked vectors finish before anybody may free or refill them)
      if (arith_may_degrade(*m) && attempt == 0) {
        arith_degrade(*m, "an activation left float16's range (non-finite edge gradient on the f16x2 arithmetic); the evaluation was repeated");
        continue;
      }
      throw StateError("fused_arith=f16x2: an edge gradient was not finite (an activation left float16's range, or the input was not finite): the forces of this "
                       "evaluation are invalid and were not added to f; set option fused_arith=f32 (or auto) for this model");
    }
    break;
    }
    // scatter: f[i] += forces[i] for locals AND ghosts (pair_nequip_allegro.cpp:370-377)
    {
      const double *const hf = m->h_f.data();
      for (size_t c = 0; c < nfch; ++c) {
        AHIP_CHECK(hipEventSynchronize(m->f_events[c]));
        const size_t k0 = c * (FCH / sizeof(double)), k1 = std::min((size_t)nall * 3, k0 + FCH / sizeof(double));
        parallel_for(k1 - k0, [=](size_t b, size_t e) { for (size_t k = k0 + b; k < k0 + e; ++k) f[k] += hf[k]; });
      }
    }
    AHIP_CHECK(hipStreamSynchronize(s));
    if (eatom) {
      const double *const he = m->h_eatom.data();
      const int *const il = m->h_ilist.empty() ? nullptr : m->h_ilist.data();
      parallel_for((size_t)m->inum, [=](size_t b, size_t e) { for (size_t ii = b; ii < e; ++ii) { const int i = il ? il[ii] : (int)ii; eatom[i] = he[i]; } });
    }
    *eng = ev[0];
    if (virial) for (int k = 0; k < 6; ++k) virial[k] = ev[1 + k];
    if (!m->custom_names.empty()) store_custom_outputs(m, nall, m->inum, m->h_ilist.empty() ? nullptr : m->h_ilist.data(), ev);
  });
}

int ahip_output_register(ahip_model *m, const char *name) {
  return guarded([&] {
    require_model(m);
    if (!name || !*name) throw ArgError("ahip_output_register: empty name");
    m->custom_names.push_back(name);
  });
}

int ahip_output_get(ahip_model *m, const char *name, double *out, long long capacity, long long *count) {
  return guarded([&] {
    require_model(m);
    if (!name || !count) throw ArgError("ahip_output_get: NULL name/count");
    auto it = m->custom_out.find(name);
    if (it == m->custom_out.end())
      throw StateError(std::string("output '") + name + "' is not stored: register it with ahip_output_register before ahip_compute / "
                       "ahip_compute_dev (nlocal > 0)");
    *count = (long long)it->second.size();
    if (!out) return;
    if (capacity < *count) throw ArgError("ahip_output_get: buffer too small");
    std::copy(it->second.begin(), it->second.end(), out);
  });
}

int ahip_compute_dev(ahip_model *m, int nlocal, int nghost, const double *x_dev, const int *mtype_dev,
                     const double *cutoff_matrix_model, double *f_dev, double *eatom_dev, double *eng_vir_dev,
                     void *stream) {
  return guarded([&] {
    require_model(m);
    if (!m->have_list) throw StateError("ahip_compute_dev called before a neighbor list was installed");
    const int nall = nlocal + nghost;
    if (nall != m->nall) throw StateError("ahip_compute_dev: nlocal+nghost differs from the neighbor list's nall");
    if (!x_dev || !mtype_dev || !f_dev || !eng_vir_dev) throw ArgError("ahip_compute_dev: NULL device pointer");
    AHIP_CHECK(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    const int T = m->hm.num_types;
    std::vector<double> cutsq((size_t)T * T);
    for (size_t k = 0; k < cutsq.size(); ++k) {
      double c = cutoff_matrix_model ? cutoff_matrix_model[k] : m->rcut_model_host[k];
      cutsq[k] = cutsq_bound(m, c);
    }
    if (cutsq != m->h_cutsq_dev) {                           // upload (and synchronise) only when the matrix changes
      m->b_cutsq.reserve(cutsq.size() * sizeof(double));
      AHIP_CHECK(hipMemcpyAsync(m->b_cutsq.p, cutsq.data(), cutsq.size() * sizeof(double), hipMemcpyHostToDevice, s));
      AHIP_CHECK(hipStreamSynchronize(s));                   // cutsq is a stack vector
      m->h_cutsq_dev = cutsq;
    }
    if (m->custom_names.empty()) {
      ComputeArgs a{nlocal, nghost, x_dev, mtype_dev, m->b_cutsq.as<double>(), T, mtype_dev, f_dev, eatom_dev, eng_vir_dev, s};
      run_model(m, a);
    } else {
      // `compute allegro` on the device path (the reference's Kokkos class keeps output.at(name) too,
      // pair_nequip_allegro_kokkos.cpp:342-344): evaluate into the library's own zeroed force / energy arrays, add them to the
      // caller's, and keep host copies of the named entries.  Costs two extra array passes and a read-back, only when a
      // compute is registered.
      check_output_names(m);
      double *vatom = want_atomic_virial(m) ? vatom_buffer(m, nall) : nullptr;
      m->b_f.reserve((size_t)std::max(nall, 1) * 3 * sizeof(double));
      m->b_eatom.reserve((size_t)std::max(nall, 1) * sizeof(double));
      AHIP_CHECK(hipMemsetAsync(m->b_f.p, 0, (size_t)nall * 3 * sizeof(double), s));
      AHIP_CHECK(hipMemsetAsync(m->b_eatom.p, 0, (size_t)nall * sizeof(double), s));
      ComputeArgs a{nlocal, nghost, x_dev, mtype_dev, m->b_cutsq.as<double>(), T, mtype_dev, m->b_f.as<double>(), m->b_eatom.as<double>(), eng_vir_dev, s, vatom};
      run_model(m, a);
      const int inum = m->inum;
      if (nall > 0) hipLaunchKernelGGL(k_add_n, dim3((unsigned)((3LL * nall + 255) / 256)), dim3(256), 0, s, 3LL * nall, f_dev, m->b_f.as<double>());
      if (eatom_dev && inum > 0) hipLaunchKernelGGL(k_copy_centres, dim3((unsigned)((inum + 255) / 256)), dim3(256), 0, s, inum, m->d_ilist, eatom_dev, m->b_eatom.as<double>());
      AHIP_CHECK(hipGetLastError());
      unpin_if_growing(m, m->h_f, (size_t)nall * 3); unpin_if_growing(m, m->h_eatom, (size_t)nall); unpin_if_growing(m, m->h_mtype, (size_t)nall);
      m->h_f.resize((size_t)nall * 3); m->h_eatom.resize(nall); m->h_mtype.resize(nall);
      std::vector<int> il(inum);
      double ev[7];
      AHIP_CHECK(hipStreamSynchronize(s));
      copy_d2h(m->h_f.data(), m->b_f.p, (size_t)nall * 3 * sizeof(double));          // pageable vectors: staged (engine.h)
      copy_d2h(m->h_eatom.data(), m->b_eatom.p, (size_t)nall * sizeof(double));
      copy_d2h(m->h_mtype.data(), mtype_dev, (size_t)nall * sizeof(int));
      if (inum > 0) copy_d2h(il.data(), m->d_ilist, (size_t)inum * sizeof(int));
      copy_d2h(ev, eng_vir_dev, 7 * sizeof(double));
      store_custom_outputs(m, nall, inum, il.data(), ev);
    }
  });
}

int ahip_compute_dev_range(ahip_model *m, int centre_begin, int centre_end, int nlocal, int nghost, const double *x_dev,
                           const int *mtype_dev, const double *cutoff_matrix_model, double *f_dev, double *eatom_dev,
                           double *eng_vir_dev, void *stream) {
  return guarded([&] {
    require_model(m);
    if (!m->have_list) throw StateError("ahip_compute_dev_range called before a neighbor list was installed");
    if (centre_begin < 0 || centre_end < centre_begin || centre_end > m->inum)
      throw ArgError("ahip_compute_dev_range: need 0 <= centre_begin <= centre_end <= inum");
    if (!m->custom_names.empty()) throw StateError("ahip_compute_dev_range: registered model outputs (compute allegro) need the whole-list call ahip_compute_dev");
    // narrow the installed CSR list to the centre range (offsets are absolute into the neighbour array), evaluate, restore
    const int inum = m->inum;
    const int *il = m->d_ilist, *off = m->d_nloff;
    m->d_ilist = il + centre_begin; m->d_nloff = off + centre_begin; m->inum = centre_end - centre_begin;
    const int rc = ahip_compute_dev(m, nlocal, nghost, x_dev, mtype_dev, cutoff_matrix_model, f_dev, eatom_dev, eng_vir_dev, stream);
    const std::string err = g_err;
    m->d_ilist = il; m->d_nloff = off; m->inum = inum;
    if (rc == AHIP_ERR_ARG) throw ArgError(err);
    if (rc == AHIP_ERR_STATE) throw StateError(err);
    if (rc == AHIP_ERR_UNSUPPORTED) throw UnsupportedError(err);
    if (rc != AHIP_OK) throw HipError(err);
  });
}

long long ahip_last_list_size(ahip_model *m) { return m ? m->nneigh : 0; }

int ahip_get_edges(ahip_model *m, long long *nedges, long long *edge_index, double *rij) {
  return guarded([&] {
    require_model(m);
    if (!nedges) throw ArgError("ahip_get_edges: nedges is NULL");
    edges_counts(*m);
    fused_poll_alarm(*m);                    // (an accessor that waits for the device also reports an alarm nobody has collected)
    *nedges = m->nedges;
    if (!edge_index && !rij) return;
    const size_t E = (size_t)m->nedges;
    if (E == 0) return;
    AHIP_CHECK(hipSetDevice(m->device));
    AHIP_CHECK(hipDeviceSynchronize());
    std::vector<int> eii(E), ej(E), il(m->inum);
    copy_d2h(eii.data(), m->b_eii.p, E * sizeof(int));
    copy_d2h(ej.data(), m->b_ej.p, E * sizeof(int));
    copy_d2h(il.data(), m->d_ilist, (size_t)m->inum * sizeof(int));
    if (edge_index)
      for (size_t e = 0; e < E; ++e) { edge_index[e] = il[eii[e]]; edge_index[E + e] = ej[e]; }
    if (rij) {
      if (m->edges_T_size == 8) {
        std::vector<double> r(E * 3);
        copy_d2h(r.data(), m->b_rvec.p, E * 3 * sizeof(double));
        for (size_t e = 0; e < E; ++e) rij[e] = std::sqrt(r[3 * e] * r[3 * e] + r[3 * e + 1] * r[3 * e + 1] + r[3 * e + 2] * r[3 * e + 2]);
      } else {
        std::vector<float> r(E * 3);
        copy_d2h(r.data(), m->b_rvec.p, E * 3 * sizeof(float));
        for (size_t e = 0; e < E; ++e) {
          double a = r[3 * e], b = r[3 * e + 1], c = r[3 * e + 2];
          rij[e] = std::sqrt(a * a + b * b + c * c);
        }
      }
    }
  });
}

int ahip_debug_dump_edges(ahip_model *m, const int *tag) {
  return guarded([&] {
    require_model(m);
    long long E = 0;
    std::vector<long long> ei;
    std::vector<double> r;
    if (ahip_get_edges(m, &E, nullptr, nullptr) != AHIP_OK) throw std::runtime_error(g_err);
    ei.resize((size_t)2 * E); r.resize((size_t)E);
    if (E > 0 && ahip_get_edges(m, &E, ei.data(), r.data()) != AHIP_OK) throw std::runtime_error(g_err);
    // exact format of pair_nequip_allegro.cpp:564,625,632
    std::printf("Allegro edges: i j rij\n");
    for (long long e = 0; e < E; ++e) {
      long long i = ei[e], j = ei[E + e];
      if (tag) std::printf("%d %d %.10g\n", tag[i] - 1, tag[j] - 1, r[e]);
      else std::printf("%lld %lld %.10g\n", i, j, r[e]);
    }
    std::printf("end Allegro edges\n");
    std::fflush(stdout);
  });
}

int ahip_get_timings(ahip_model *m, const char **names, const double **ms, int *n) {
  return guarded([&] {
    require_model(m);
    AHIP_CHECK(hipSetDevice(m->device));
    collect_timings(m);
    fused_poll_alarm(*m);
    if (names) *names = m->timing_names.c_str();
    if (ms) *ms = m->timing_ms.data();
    if (n) *n = (int)m->timing_ms.size();
  });
}
int ahip_get_timing_counts(ahip_model *m, const double **counts, int *n) {
  return guarded([&] {
    require_model(m);
    if (counts) *counts = m->timing_counts.data();
    if (n) *n = (int)m->timing_counts.size();
  });
}

// Diagnostics: edge slots of the tiles of the last fused evaluation and how many of them held an edge (the padding tax of the tile packing:
// bulk Si 0.875, Li3PO4 ~0.77, water ~0.82).  Reads two device words (synchronises the default stream); 0 / 0 when the last path was not a fused one.
extern "C" int ahip_last_tile_occupancy(ahip_model *m, long long *slots_used, long long *slots_total) {
  return guarded([&] {
    require_model(m);
    if (!slots_used || !slots_total) throw ArgError("ahip_last_tile_occupancy: NULL argument");
    *slots_used = 0; *slots_total = 0;
    if (!m->d_ntiles_last || m->last_path.rfind("fused", 0) != 0) return;
    AHIP_CHECK(hipSetDevice(m->device));
    AHIP_CHECK(hipDeviceSynchronize());        // the tile count may come from the stand-alone packing kernels on a non-blocking stream: a null-stream copy does not wait for those
    edges_counts(*m);
    int nt = 0;
    AHIP_CHECK(hipMemcpy(&nt, m->d_ntiles_last, sizeof(int), hipMemcpyDeviceToHost));
    const int slots = m->last_tile_slots ? m->last_tile_slots : (m->last_max_deg <= 64 ? 64 : 128);
    *slots_used = m->last_tile_edges >= 0 ? m->last_tile_edges : m->nedges;      // (dense_centres=split behind the two-pass edge build: the tiles hold the light centres only)
    *slots_total = (long long)nt * slots;
  });
}

// last kernel family used ("generic_f32" | "generic_f64" | "fused_f32" | "fused_tf32eq")
extern "C" const char *ahip_last_path(ahip_model *m) { return m ? m->last_path.c_str() : ""; }
// what fused_arith=auto decided for this model and why (empty until the first evaluation): "f16x2 kept: ..." or "float32 instance selected: ..."
extern "C" const char *ahip_arith_note(const ahip_model *m) { return m ? m->arith.note.c_str() : ""; }
extern "C" int ahip_last_max_degree(ahip_model *m) {
  if (!m) return 0;
  if (guarded([&] { edges_counts(*m); }) != 0) return -1;
  return m->last_max_deg;
}

int ahip_last_heavy_centres(ahip_model *m, int *ncentres, long long *nedges) {
  return guarded([&] {
    require_model(m);
    if (!ncentres || !nedges) throw ArgError("ahip_last_heavy_centres: NULL argument");
    edges_counts(*m);
    *ncentres = m->last_heavy_centres; *nedges = m->last_heavy_edges;
  });
}

int ahip_build_neighbors_dev(ahip_model *m, int nlocal, int nall, const double *x_dev, const double *lo,
                             const double *hi, double rc_list, void *stream) {
  return guarded([&] {
    require_model(m);
    if (nlocal < 0 || nall < nlocal) throw ArgError("ahip_build_neighbors_dev: need 0 <= nlocal <= nall");
    if (!x_dev || !lo || !hi || !(rc_list > 0)) throw ArgError("ahip_build_neighbors_dev: bad argument");
    AHIP_CHECK(hipSetDevice(m->device));
    neigh_build(*m, nlocal, nall, x_dev, lo, hi, rc_list, (hipStream_t)stream);
  });
}

int ahip_neigh_update_dev_table(ahip_model *m, int inum, int nall, const int *ilist_dev, const int *numneigh_dev,
                                const int *neighbors_dev, long long stride_atom, long long stride_slot, int neighmask, void *stream) {
  return guarded([&] {
    require_model(m);
    check_list_dims(inum, nall);
    if (inum > 0 && (!ilist_dev || !numneigh_dev || !neighbors_dev)) throw ArgError("ahip_neigh_update_dev_table: NULL list pointer");
    if (stride_atom < 1 || stride_slot < 1) throw ArgError("ahip_neigh_update_dev_table: strides must be positive");
    AHIP_CHECK(hipSetDevice(m->device));
    neigh_from_table(*m, inum, nall, ilist_dev, numneigh_dev, neighbors_dev, stride_atom, stride_slot, neighmask, (hipStream_t)stream);
  });
}

int ahip_map_types_dev(ahip_model *m, int n, const int *type_dev, int ntypes, const int *type_mapper, int *mtype_dev, void *stream) {
  return guarded([&] {
    require_model(m);
    if (n < 0 || ntypes < 1 || !type_mapper || (n > 0 && (!type_dev || !mtype_dev))) throw ArgError("ahip_map_types_dev: bad argument");
    AHIP_CHECK(hipSetDevice(m->device));
    m->active_mapped = mapped_types(*m, ntypes, type_mapper);
    map_types(*m, n, type_dev, ntypes, type_mapper, mtype_dev, (hipStream_t)stream);
  });
}

int ahip_set_active_types(ahip_model *m, int n, const int *model_types) {
  return guarded([&] {
    require_model(m);
    if (n < 0 || (n > 0 && !model_types)) throw ArgError("ahip_set_active_types: bad argument");
    std::vector<int> v(model_types, model_types + n);
    for (int t : v)
      if (t < 0 || t >= m->hm.num_types) throw ArgError("ahip_set_active_types: model type " + std::to_string(t) + " is outside the model's " + std::to_string(m->hm.num_types) + " types");
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    m->active_set = v;                       // installed by the next evaluation (run_model: resolve_active)
  });
}

int ahip_get_active_types(ahip_model *m, int *n, int *model_types) {
  return guarded([&] {
    require_model(m);
    if (!n) throw ArgError("ahip_get_active_types: n is NULL");
    fused_poll_alarm(*m);                    // (an inactive type met by the last device-resident evaluation is reported here at the latest)
    *n = (int)m->active.size();
    if (model_types) std::copy(m->active.begin(), m->active.end(), model_types);
  });
}

int ahip_reneighbor_flag_dev(ahip_model *m, int n, const double *x_dev, const double *xhold_dev, const double *v_dev, double dt,
                             double half_skin, int *flag_dev, void *stream) {
  return guarded([&] {
    require_model(m);
    if (n < 0 || !flag_dev || (n > 0 && (!x_dev || !xhold_dev || !v_dev))) throw ArgError("ahip_reneighbor_flag_dev: bad argument");
    AHIP_CHECK(hipSetDevice(m->device));
    if (!m->b_flagwork.p) { m->b_flagwork.reserve(64); AHIP_CHECK(hipMemsetAsync(m->b_flagwork.p, 0, 64, (hipStream_t)stream)); }      // the two maxima start from zero; the flag kernel resets them after every use
    AHIP_CHECK(prim_reneighbor_flag(x_dev, xhold_dev, v_dev, n, dt, half_skin, m->b_flagwork.as<unsigned int>(), flag_dev, (hipStream_t)stream));
  });
}

int ahip_borders_local_dev(ahip_model *m, int nlocal, const double *x_dev, const int *mtype_dev, const double *lo, const double *hi, const double *box, double rc,
                           int capacity, double *xg_dev, int *mtg_dev, long long *src_dev, double *shift_dev, int *nghost, void *stream) {
  return guarded([&] {
    require_model(m);
    if (nlocal < 0 || capacity < 0 || !lo || !hi || !box || !nghost || !(rc > 0.0) || (nlocal > 0 && (!x_dev || !mtype_dev)) ||
        (capacity > 0 && (!xg_dev || !mtg_dev || !src_dev || !shift_dev)))
      throw ArgError("ahip_borders_local_dev: bad argument");
    AHIP_CHECK(hipSetDevice(m->device));
    *nghost = borders_local(*m, nlocal, x_dev, mtype_dev, lo, hi, box, rc, capacity, xg_dev, mtg_dev, src_dev, shift_dev, (hipStream_t)stream);
  });
}

int ahip_wrap_cell_dev(ahip_model *m, int n, double *x_dev, const double *cell, const int *pbc, void *stream) {
  return guarded([&] {
    require_model(m);
    if (n < 0 || !cell || !pbc || (n > 0 && !x_dev)) throw ArgError("ahip_wrap_cell_dev: bad argument");
    AHIP_CHECK(hipSetDevice(m->device));
    wrap_cell(*m, n, x_dev, cell, pbc, (hipStream_t)stream);
  });
}

int ahip_borders_cell_dev(ahip_model *m, int nlocal, const double *x_dev, const int *mtype_dev, const double *cell, const int *pbc, double rc, int capacity,
                          double *xg_dev, int *mtg_dev, long long *src_dev, double *shift_dev, int *nghost, void *stream) {
  return guarded([&] {
    require_model(m);
    if (nlocal < 0 || capacity < 0 || !cell || !pbc || !nghost || !(rc > 0.0) || !std::isfinite(rc) || (nlocal > 0 && (!x_dev || !mtype_dev)) ||
        (capacity > 0 && (!xg_dev || !mtg_dev || !src_dev || !shift_dev)))
      throw ArgError("ahip_borders_cell_dev: bad argument");
    AHIP_CHECK(hipSetDevice(m->device));
    *nghost = borders_cell(*m, nlocal, x_dev, mtype_dev, cell, pbc, rc, capacity, xg_dev, mtg_dev, src_dev, shift_dev, (hipStream_t)stream);
  });
}

// the error of a nested C-ABI call, thrown again as what it was
static void rethrow_code(int rc) {
  if (rc == AHIP_OK) return;
  const std::string err = g_err;
  if (rc == AHIP_ERR_ARG) throw ArgError(err);
  if (rc == AHIP_ERR_STATE) throw StateError(err);
  if (rc == AHIP_ERR_UNSUPPORTED) throw UnsupportedError(err);
  throw HipError(err);
}

// what ahip_compute_cell and ahip_compute_cell_reuse refuse alike, before anything is written or launched; returns the model types present
static std::vector<int> cell_check_args(const ahip_model *m, const std::string &who, int natoms, const double *x, const int *mtype, const double *cell, const int *pbc,
                                        double skin, const double *f, const double *eng) {
  if (natoms < 0 || !cell || !pbc || !eng || (natoms > 0 && (!x || !mtype || !f))) throw ArgError(who + ": bad argument");
  if (!(skin >= 0.0) || !std::isfinite(skin)) throw ArgError(who + ": skin must be a finite number >= 0");
  const int T = m->hm.num_types;
  std::vector<int> present;
  for (int i = 0; i < natoms; ++i) {
    if (mtype[i] < 0 || mtype[i] >= T)
      throw ArgError(who + ": atom " + std::to_string(i) + " has model type " + std::to_string(mtype[i]) + ", outside the model's " + std::to_string(T) + " types");
    present.push_back(mtype[i]);
  }
  std::sort(present.begin(), present.end());
  present.erase(std::unique(present.begin(), present.end()), present.end());
  return present;
}

// One evaluation on the rows of c_x / c_mtype with the installed list, enqueued: zeroed f and eatom, ahip_compute_dev, ghost forces folded home (newton on)
static void cell_evaluate_enqueue(ahip_model *m, int natoms, int ng, hipStream_t s) {
  const int nall = natoms + ng;
  AHIP_CHECK(hipMemsetAsync(m->c_f.p, 0, (size_t)std::max(nall, 1) * 3 * sizeof(double), s));
  AHIP_CHECK(hipMemsetAsync(m->c_eatom.p, 0, (size_t)std::max(nall, 1) * sizeof(double), s));
  rethrow_code(ahip_compute_dev(m, natoms, ng, m->c_x.as<double>(), m->c_mtype.as<int>(), nullptr, m->c_f.as<double>(), m->c_eatom.as<double>(),
                                m->c_engvir.as<double>(), s));
  comm_scatter_local(ng, natoms, m->c_src.as<long long>(), m->c_f.as<double>(), s);
  AHIP_CHECK(hipGetLastError());
}
// The evaluation with its one synchronisation; the results stay on the device.  Returns how many evaluations it took
// (twice at most: an evaluation whose f16x2 kernels raise the float16-range alarm under fused_arith=auto is repeated on the float32 instance, as in ahip_compute)
static int cell_evaluate_dev(ahip_model *m, const std::string &who, int natoms, int ng, hipStream_t s) {
  for (int attempt = 0;; ++attempt) {
    cell_evaluate_enqueue(m, natoms, ng, s);
    AHIP_CHECK(hipStreamSynchronize(s));
    if (const int bad = inactive_take(*m)) throw ArgError(who + ": " + inactive_message(*m, bad, "this evaluation") + " (nothing was written to f)");
    if (alarm_take(*m)) {
      if (arith_may_degrade(*m) && attempt == 0) {
        arith_degrade(*m, "an activation left float16's range (non-finite edge gradient on the f16x2 arithmetic); the evaluation was repeated");
        continue;
      }
      throw StateError("fused_arith=f16x2: an edge gradient was not finite (an activation left float16's range, or the input was not finite): the forces of this "
                       "evaluation are invalid and were not written to f; set option fused_arith=f32 (or auto) for this model");
    }
    return attempt + 1;
  }
}
// the downloads of an evaluation that has been waited for
static void cell_download(ahip_model *m, int natoms, double *f, double *eatom, double *eng, double *virial) {
  double ev[7];
  copy_d2h(ev, m->c_engvir.p, 7 * sizeof(double));
  if (natoms > 0) {
    copy_d2h(f, m->c_f.p, (size_t)natoms * 3 * sizeof(double));
    if (eatom) copy_d2h(eatom, m->c_eatom.p, (size_t)natoms * sizeof(double));
  }
  *eng = ev[0];
  if (virial) for (int k = 0; k < 6; ++k) virial[k] = ev[1 + k];
}
static void cell_evaluate(ahip_model *m, const std::string &who, int natoms, int ng, double *f, double *eatom, double *eng, double *virial, hipStream_t s) {
  cell_evaluate_dev(m, who, natoms, ng, s);
  cell_download(m, natoms, f, eatom, eng, virial);
}

// Rows and list of a cell: positions in (from the host, or with x_on_device from device memory), wrap, ghosts, neighbor list.  Returns the number of ghosts.
static int cell_rows(ahip_model *m, const std::string &who, const std::vector<int> &present, int natoms, const double *x, bool x_on_device, const int *mtype,
                     const double *cell, const int *pbc, double skin) {
  const double rc = *std::max_element(m->rcut_model_host.begin(), m->rcut_model_host.end()) + skin;
  AHIP_CHECK(hipSetDevice(m->device));
  hipStream_t s = nullptr;
  m->hold.serial = 0;                         // the rows of a held list are overwritten from here on
  // upload, wrap, ghosts: rows [0, natoms) of c_x / c_mtype are the atoms, the images go behind them.  The first capacity is the last call's count when the
  // system has the same size, else none (the call then only counts); a grown buffer loses its content, so the one retry uploads again
  int cap = natoms == m->cell_natoms ? m->cell_nghost_last + m->cell_nghost_last / 8 : 0, ng = 0;
  m->cell_src_host.clear(); m->cell_natoms = natoms;
  double lo[3], hi[3];
  cell_bounding_box(cell, rc + 1e-6, lo, hi);
  for (;;) {
    const size_t rows = (size_t)natoms + (size_t)cap;
    m->c_x.reserve(std::max<size_t>(rows, 1) * 3 * sizeof(double));
    m->c_mtype.reserve(std::max<size_t>(rows, 1) * sizeof(int));
    m->c_src.reserve(std::max<size_t>((size_t)cap, 1) * sizeof(long long));
    m->c_shift.reserve(std::max<size_t>((size_t)cap, 1) * 3 * sizeof(double));
    if (natoms > 0) {
      if (x_on_device) AHIP_CHECK(hipMemcpyAsync(m->c_x.p, x, (size_t)natoms * 3 * sizeof(double), hipMemcpyDeviceToDevice, s));
      else copy_h2d(m->c_x.p, x, (size_t)natoms * 3 * sizeof(double));
      copy_h2d(m->c_mtype.p, mtype, (size_t)natoms * sizeof(int));
    }
    wrap_cell(*m, natoms, m->c_x.as<double>(), cell, pbc, s);
    ng = borders_cell(*m, natoms, m->c_x.as<double>(), m->c_mtype.as<int>(), cell, pbc, rc, cap, m->c_x.as<double>() + 3 * (size_t)natoms,
                      m->c_mtype.as<int>() + natoms, m->c_src.as<long long>(), m->c_shift.as<double>(), s);
    if (ng <= cap) break;
    cap = ng;
  }
  m->cell_nghost_last = ng;
  if ((long long)natoms + ng > 2147483647LL) throw ArgError(who + ": atoms + ghosts exceed 2^31 - 1 rows");
  const int nall = natoms + ng;
  m->cell_src_host.resize((size_t)ng);
  if (ng > 0) copy_d2h(m->cell_src_host.data(), m->c_src.p, (size_t)ng * sizeof(long long));
  m->active_mapped = present;               // a model of more than 16 types runs on the types present (run_model: resolve_active)
  neigh_build(*m, natoms, nall, m->c_x.as<double>(), lo, hi, rc, s);
  m->c_f.reserve((size_t)std::max(nall, 1) * 3 * sizeof(double));
  m->c_eatom.reserve((size_t)std::max(nall, 1) * sizeof(double));
  m->c_engvir.reserve(8 * sizeof(double));
  return ng;
}
// ahip_compute_cell, and the rebuild path of ahip_compute_cell_reuse: upload, wrap, ghosts, list, evaluation, download.  Returns the number of ghosts.
static int cell_rebuild(ahip_model *m, const std::string &who, const std::vector<int> &present, int natoms, const double *x, const int *mtype, const double *cell,
                        const int *pbc, double skin, double *f, double *eatom, double *eng, double *virial) {
  *eng = 0;
  if (virial) for (int k = 0; k < 6; ++k) virial[k] = 0;
  const int ng = cell_rows(m, who, present, natoms, x, false, mtype, cell, pbc, skin);
  cell_evaluate(m, who, natoms, ng, f, eatom, eng, virial, nullptr);
  return ng;
}

int ahip_compute_cell(ahip_model *m, int natoms, const double *x, const int *mtype, const double *cell, const int *pbc, double skin, double *f,
                      double *eatom, double *eng, double *virial) {
  return guarded([&] {
    require_model(m);
    const std::vector<int> present = cell_check_args(m, "ahip_compute_cell", natoms, x, mtype, cell, pbc, skin, f, eng);
    cell_rebuild(m, "ahip_compute_cell", present, natoms, x, mtype, cell, pbc, skin, f, eatom, eng, virial);
  });
}

int ahip_compute_cell_reuse(ahip_model *m, int natoms, const double *x, const int *mtype, const double *cell, const int *pbc, double skin, double *f,
                            double *eatom, double *eng, double *virial, int *rebuilt) {
  return guarded([&] {
    require_model(m);
    const std::string who = "ahip_compute_cell_reuse";
    const std::vector<int> present = cell_check_args(m, who, natoms, x, mtype, cell, pbc, skin, f, eng);
    (void)cell_geometry(who.c_str(), cell, pbc, 1.0);      // a singular or non-finite cell is refused here, with the hold as it was
    const Model::CellHold &h = m->hold;
    bool held = skin > 0.0 && h.serial != 0 && h.serial == m->list_serial && natoms == h.natoms && skin == h.skin;
    for (int d = 0; held && d < 3; ++d) held = (pbc[d] != 0) == (h.pbc[d] != 0);
    held = held && std::equal(mtype, mtype + natoms, h.mtype.begin());
    // Whatever fails from here on fails behind a launch and leaves nothing held; a success restores the hold or replaces it.
    const unsigned long long serial = h.serial;
    m->hold.serial = 0;
    AHIP_CHECK(hipSetDevice(m->device));
    hipStream_t s = nullptr;
    if (held && cell_hold_refresh(*m, x, cell, s)) {
      *eng = 0;
      if (virial) for (int k = 0; k < 6; ++k) virial[k] = 0;
      if (m->cell_natoms != natoms || (int)m->cell_src_host.size() != h.nghost) {      // (a batch without atoms in between has reset what ahip_last_cell_rows reports)
        m->cell_natoms = natoms; m->cell_nghost_last = h.nghost;
        m->cell_src_host.resize((size_t)h.nghost);
        if (h.nghost > 0) copy_d2h(m->cell_src_host.data(), m->c_src.p, (size_t)h.nghost * sizeof(long long));
      }
      m->active_mapped = present;
      cell_evaluate(m, who, natoms, h.nghost, f, eatom, eng, virial, s);
      m->hold.serial = serial;
      if (rebuilt) *rebuilt = 0;
    } else {
      const int ng = cell_rebuild(m, who, present, natoms, x, mtype, cell, pbc, skin, f, eatom, eng, virial);
      const double rc = *std::max_element(m->rcut_model_host.begin(), m->rcut_model_host.end()) + skin;
      cell_hold_take(*m, natoms, ng, cell, pbc, skin, rc, s);
      m->hold.mtype.assign(mtype, mtype + natoms);
      m->hold.serial = m->list_serial;
      ++m->reuse_rebuilds;
      if (rebuilt) *rebuilt = 1;
    }
    ++m->reuse_calls;
  });
}

int ahip_cell_reuse_reset(ahip_model *m) {
  return guarded([&] {
    require_model(m);
    m->hold.serial = 0;
    m->reuse_calls = m->reuse_rebuilds = 0;
  });
}

int ahip_cell_reuse_stats(ahip_model *m, long long *calls, long long *rebuilds) {
  return guarded([&] {
    require_model(m);
    if (calls) *calls = m->reuse_calls;
    if (rebuilds) *rebuilds = m->reuse_rebuilds;
  });
}

int ahip_relax_params_default(ahip_relax_params *p) {
  return guarded([&] {
    if (!p) throw ArgError("ahip_relax_params_default: p is NULL");
    *p = ahip_relax_params{0.05, 500, 4, 0.1, 1.0, 0.2, 5, 1.1, 0.5, 0.1, 0.99};
  });
}

// the ranges of ahip_relax_params (include/allegro_hip.h)
static void relax_check_params(const std::string &who, const ahip_relax_params *p) {
  const auto finite_in = [](double v, double lo, double hi) { return std::isfinite(v) && v >= lo && v <= hi; };
  if (!finite_in(p->fmax, 0.0, INFINITY)) throw ArgError(who + ": fmax must be a finite number >= 0");
  if (p->max_steps < 0) throw ArgError(who + ": max_steps must be >= 0");
  if (p->check_every < 1) throw ArgError(who + ": check_every must be >= 1");
  if (!finite_in(p->dt_start, 0.0, INFINITY) || !(p->dt_start > 0.0) || !finite_in(p->dt_max, p->dt_start, INFINITY))
    throw ArgError(who + ": need 0 < dt_start <= dt_max, both finite");
  if (!finite_in(p->max_step, 0.0, INFINITY) || !(p->max_step > 0.0)) throw ArgError(who + ": max_step must be a finite number > 0");
  if (p->n_min < 0) throw ArgError(who + ": n_min must be >= 0");
  if (!finite_in(p->f_inc, 1.0, INFINITY)) throw ArgError(who + ": f_inc must be a finite number >= 1");
  if (!finite_in(p->f_dec, 0.0, 1.0) || !(p->f_dec > 0.0)) throw ArgError(who + ": f_dec must be in (0, 1]");
  if (!finite_in(p->alpha_start, 0.0, 1.0)) throw ArgError(who + ": alpha_start must be in [0, 1]");
  if (!finite_in(p->f_alpha, 0.0, 1.0) || !(p->f_alpha > 0.0)) throw ArgError(who + ": f_alpha must be in (0, 1]");
}

// FIRE at fixed cell with the optimiser's state on the device (algorithm and statuses: include/allegro_hip.h; kernels: neigh.hip).  Nothing of the caller's is
// written before the last read-back has succeeded.
int ahip_relax_cell(ahip_model *m, int natoms, double *x, const int *mtype, const double *cell, const int *pbc, double skin, const int *fixed,
                    const ahip_relax_params *p, double *f, double *eatom, double *eng, double *virial, int *steps, int *converged, double *fmax_out,
                    int *evaluations, int *rebuilds) {
  return guarded([&] {
    require_model(m);
    const std::string who = "ahip_relax_cell";
    const std::vector<int> present = cell_check_args(m, who, natoms, x, mtype, cell, pbc, skin, f, eng);
    if (!(skin > 0.0)) throw ArgError(who + ": skin must be > 0 (the skin is what the atoms may move through before the list is rebuilt)");
    if (!p) throw ArgError(who + ": p is NULL (ahip_relax_params_default fills one)");
    relax_check_params(who, p);
    (void)cell_geometry(who.c_str(), cell, pbc, 1.0);      // a singular or non-finite cell is refused here, with the hold as it was
    // Whatever fails from here on fails behind a launch and leaves nothing held.
    m->hold.serial = 0;
    AHIP_CHECK(hipSetDevice(m->device));
    hipStream_t s = nullptr;
    const double rc = *std::max_element(m->rcut_model_host.begin(), m->rcut_model_host.end()) + skin;
    const RelaxFire fire{p->fmax, p->dt_max, p->max_step, p->f_inc, p->f_dec, p->alpha_start, p->f_alpha, skin, p->n_min};
    int moves = 0, nev = 0, nreb = 0, ng = 0;
    relax_begin(*m, natoms, x, fixed, p->dt_start, p->alpha_start, s);
    // rows, list and hold from the positions on the device (those of the last move), then their forces
    const auto rebuild = [&] {
      ng = cell_rows(m, who, present, natoms, m->q_x[moves & 1].as<double>(), true, mtype, cell, pbc, skin);
      cell_hold_take(*m, natoms, ng, cell, pbc, skin, rc, s);
      relax_rows_fresh(*m, natoms, s);
      nev += cell_evaluate_dev(m, who, natoms, ng, s);
      ++nreb;
    };
    rebuild();
    bool may_repeat = true;                   // NONFINITE or the alarm: once, under fused_arith=auto, the frozen positions are evaluated again on the float32 instance
    while (natoms > 0 && moves < p->max_steps) {
      const int chunk = std::min(p->check_every, p->max_steps - moves);
      for (int k = 0; k < chunk; ++k) {       // no wait in here
        relax_step(*m, (moves + k) & 1, fire, s);
        cell_evaluate_enqueue(m, natoms, ng, s);
        ++nev;
      }
      const RelaxState st = relax_read(*m, s);
      moves = st.moves;
      if (const int bad = inactive_take(*m)) throw ArgError(who + ": " + inactive_message(*m, bad, "this evaluation") + " (nothing was written to x or f)");
      if (alarm_take(*m) || st.status == RELAX_NONFINITE) {
        if (!(arith_may_degrade(*m) && may_repeat && m->last_path.find("f16x2") != std::string::npos))      // (no other arithmetic has a float32 instance to fall back to)
          throw StateError(who + ": a force, a sum over the atoms or a displacement was not finite after " + std::to_string(moves) + " moves (coincident atoms, an input that was "
                           "not finite, or an activation left float16's range): the forces of this evaluation are invalid and nothing was written to x or f" +
                           (arith_effective(m->arith.opt) == ArithOpt::F16x2 ? "; set option fused_arith=f32 (or auto) for this model" : ""));
        may_repeat = false;
        arith_degrade(*m, "a relaxation met a non-finite force or the float16-range alarm; the positions of its last valid move were evaluated again");
        if (st.status != RELAX_NEED_REBUILD) {
          nev += cell_evaluate_dev(m, who, natoms, ng, s);
          relax_resume(*m, s);
          continue;
        }
      }
      if (st.status == RELAX_CONVERGED) break;
      if (st.status == RELAX_NEED_REBUILD) {
        rebuild();
        relax_resume(*m, s);
      }
    }
    AHIP_CHECK(hipStreamSynchronize(s));
    AHIP_CHECK(hipGetLastError());
    if (natoms > 0) copy_d2h(x, m->q_x[moves & 1].p, (size_t)natoms * 3 * sizeof(double));
    cell_download(m, natoms, f, eatom, eng, virial);
    double f2max = 0.0;                        // of the free atoms, from the forces handed out
    for (int i = 0; i < natoms; ++i)
      if (!(fixed && fixed[i])) f2max = std::max(f2max, f[3 * i] * f[3 * i] + f[3 * i + 1] * f[3 * i + 1] + f[3 * i + 2] * f[3 * i + 2]);
    if (steps) *steps = moves;
    if (converged) *converged = std::sqrt(f2max) <= p->fmax ? 1 : 0;
    if (fmax_out) *fmax_out = std::sqrt(f2max);
    if (evaluations) *evaluations = nev;
    if (rebuilds) *rebuilds = nreb;
    m->hold.mtype.assign(mtype, mtype + natoms);
    m->hold.serial = m->list_serial;
  });
}

int ahip_vcell_params_default(ahip_vcell_params *p) {
  return guarded([&] {
    if (!p) throw ArgError("ahip_vcell_params_default: p is NULL");
    *p = ahip_vcell_params{ahip_relax_params{0.05, 500, 4, 0.1, 1.0, 0.2, 5, 1.1, 0.5, 0.1, 0.99}, 1e-3, 0.0, 0.0, 0, {1, 1, 1, 1, 1, 1}};
  });
}

// max_ab |W_ext,ab| / V of a virial in the cell `a`, as k_vcell_decide forms it
static double vcell_sext(const double *virial, const double *a, const ahip_vcell_params *p) {
  const double V = std::fabs(a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]));
  double w[6];
  for (int k = 0; k < 6; ++k) w[k] = virial[k] - (k < 3 ? p->pressure * V : 0.0);
  if (p->hydrostatic) {
    const double t = (w[0] + w[1] + w[2]) / 3.0;
    for (int k = 0; k < 6; ++k) w[k] = k < 3 ? t : 0.0;
  }
  double wmax = 0.0;
  for (int k = 0; k < 6; ++k) wmax = std::max(wmax, p->mask[k] ? std::fabs(w[k]) : 0.0);
  return wmax / V;
}

// FIRE over the atoms and the cell with the optimiser's state on the device (algorithm and statuses: include/allegro_hip.h; kernels: neigh.hip).  The loop is that
// of ahip_relax_cell; the cell of a rebuild is the one the state block holds.  Nothing of the caller's is written before the last read-back has succeeded.
int ahip_relax_vcell(ahip_model *m, int natoms, double *x, const int *mtype, const double *cell, const int *pbc, double skin, const int *fixed,
                     const ahip_vcell_params *p, double *cell_out, double *f, double *eatom, double *eng, double *virial, int *steps, int *converged,
                     double *fmax_out, double *smax_out, int *evaluations, int *rebuilds) {
  return guarded([&] {
    require_model(m);
    const std::string who = "ahip_relax_vcell";
    const std::vector<int> present = cell_check_args(m, who, natoms, x, mtype, cell, pbc, skin, f, eng);
    if (!(skin > 0.0)) throw ArgError(who + ": skin must be > 0 (the skin is what the atoms and the cell may move through before the list is rebuilt)");
    if (!p) throw ArgError(who + ": p is NULL (ahip_vcell_params_default fills one)");
    if (!cell_out) throw ArgError(who + ": cell_out is NULL");
    if (!(pbc[0] && pbc[1] && pbc[2])) throw ArgError(who + ": all three axes must be periodic (relax a slab with the strain mask, not with an open axis)");
    relax_check_params(who, &p->fire);
    if (!std::isfinite(p->smax) || p->smax < 0.0) throw ArgError(who + ": smax must be a finite number >= 0");
    if (!std::isfinite(p->pressure)) throw ArgError(who + ": pressure must be finite");
    if (!std::isfinite(p->cell_factor) || p->cell_factor < 0.0) throw ArgError(who + ": cell_factor must be a finite number >= 0 (0: the number of atoms)");
    (void)cell_geometry(who.c_str(), cell, pbc, 1.0);      // a singular or non-finite cell is refused here, with the hold as it was
    // Whatever fails from here on fails behind a launch and leaves nothing held.
    m->hold.serial = 0;
    AHIP_CHECK(hipSetDevice(m->device));
    hipStream_t s = nullptr;
    const double rc = *std::max_element(m->rcut_model_host.begin(), m->rcut_model_host.end()) + skin;
    VcellPar par{};
    par.fire = RelaxFire{p->fire.fmax, p->fire.dt_max, p->fire.max_step, p->fire.f_inc, p->fire.f_dec, p->fire.alpha_start, p->fire.f_alpha, skin, p->fire.n_min};
    par.smax = p->smax; par.pressure = p->pressure; par.hydrostatic = p->hydrostatic != 0;
    par.cfac = p->cell_factor > 0.0 ? p->cell_factor : (double)std::max(natoms, 1);
    for (int k = 0; k < 6; ++k) par.mask[k] = p->mask[k] != 0;
    int moves = 0, nev = 0, nreb = 0, ng = 0;
    vcell_begin(*m, natoms, x, fixed, cell, p->fire.dt_start, p->fire.alpha_start, s);
    VcellState st = vcell_read(*m, s);
    // rows, list and hold from x = D q of the last move in the cell of the state block, then their forces
    const auto rebuild = [&] {
      vcell_positions(*m, natoms, moves & 1, s);
      ng = cell_rows(m, who, present, natoms, m->q_xc.as<double>(), true, mtype, st.geom.h, pbc, skin);
      cell_hold_take(*m, natoms, ng, st.geom.h, pbc, skin, rc, s);
      relax_rows_fresh(*m, natoms, s);
      nev += cell_evaluate_dev(m, who, natoms, ng, s);
      vcell_held(*m, st, s);
      ++nreb;
    };
    rebuild();
    bool may_repeat = true;                   // NONFINITE or the alarm: once, under fused_arith=auto, the frozen configuration is evaluated again on the float32 instance
    bool checked = true;                      // the configuration on the device has passed the decisions 1-4 (or is that of a rebuild)
    while (natoms > 0 && (moves < p->fire.max_steps || !checked)) {
      const bool last = moves >= p->fire.max_steps;      // no move left: the configuration of the last move is only checked
      const int chunk = std::min(p->fire.check_every, p->fire.max_steps - moves);
      if (last) vcell_check(*m, moves & 1, par, s);
      for (int k = 0; k < chunk; ++k) {       // no wait in here
        vcell_step(*m, (moves + k) & 1, par, s);
        cell_evaluate_enqueue(m, natoms, ng, s);
        ++nev;
      }
      st = vcell_read(*m, s);
      checked = last;
      moves = st.moves;
      if (const int bad = inactive_take(*m)) throw ArgError(who + ": " + inactive_message(*m, bad, "this evaluation") + " (nothing was written to x, cell_out or f)");
      if (alarm_take(*m) || st.status == RELAX_NONFINITE) {
        if (!(arith_may_degrade(*m) && may_repeat && m->last_path.find("f16x2") != std::string::npos))      // (no other arithmetic has a float32 instance to fall back to)
          throw StateError(who + ": a force, a sum over the rows, a displacement or the cell was not finite, or the cell would invert, after " + std::to_string(moves) +
                           " moves (coincident atoms, an input that was not finite, a cell_factor too small for max_step, or an activation left float16's range): the forces "
                           "of this evaluation are invalid and nothing was written to x, cell_out or f" +
                           (arith_effective(m->arith.opt) == ArithOpt::F16x2 ? "; set option fused_arith=f32 (or auto) for this model" : ""));
        may_repeat = false;
        checked = false;
        arith_degrade(*m, "a relaxation met a non-finite force or the float16-range alarm; the configuration of its last valid move was evaluated again");
        if (st.status != RELAX_NEED_REBUILD) {
          nev += cell_evaluate_dev(m, who, natoms, ng, s);
          vcell_resume(*m, s);
          continue;
        }
      }
      if (st.status == RELAX_CONVERGED) break;
      if (st.status == RELAX_NEED_REBUILD) {
        rebuild();
        checked = true;
      }
    }
    AHIP_CHECK(hipStreamSynchronize(s));
    AHIP_CHECK(hipGetLastError());
    vcell_positions(*m, natoms, moves & 1, s);
    AHIP_CHECK(hipStreamSynchronize(s));
    if (natoms > 0) copy_d2h(x, m->q_xc.p, (size_t)natoms * 3 * sizeof(double));
    double vir[6];
    cell_download(m, natoms, f, eatom, eng, vir);
    if (virial) std::copy(vir, vir + 6, virial);
    std::copy(st.geom.h, st.geom.h + 9, cell_out);
    double f2max = 0.0;                        // of the free atoms, from the forces handed out
    for (int i = 0; i < natoms; ++i)
      if (!(fixed && fixed[i])) f2max = std::max(f2max, f[3 * i] * f[3 * i] + f[3 * i + 1] * f[3 * i + 1] + f[3 * i + 2] * f[3 * i + 2]);
    const double sext = vcell_sext(vir, cell_out, p);
    if (steps) *steps = moves;
    if (converged) *converged = std::sqrt(f2max) <= p->fire.fmax && sext <= p->smax ? 1 : 0;
    if (fmax_out) *fmax_out = std::sqrt(f2max);
    if (smax_out) *smax_out = sext;
    if (evaluations) *evaluations = nev;
    if (rebuilds) *rebuilds = nreb;
    m->hold.mtype.assign(mtype, mtype + natoms);
    m->hold.serial = m->list_serial;
  });
}

int ahip_md_params_default(ahip_md_params *p) {
  return guarded([&] {
    if (!p) throw ArgError("ahip_md_params_default: p is NULL");
    *p = ahip_md_params{0, 4, 1, 0, 0.001, 1.0 / 1.0364269e-4, 1.0364269e-4, 0.0, 0.0, 0ull, 0ull};
  });
}

// the ranges of ahip_md_params and what ahip_md_cell asks of v, mass and frames (include/allegro_hip.h); read_kT: kT is part of this run
static void md_check_args(const std::string &who, int natoms, const double *v, const double *mass, const ahip_md_params *p, const double *frames, bool read_kT) {
  const auto positive = [](double q) { return std::isfinite(q) && q > 0.0; };
  if (p->nsteps < 0) throw ArgError(who + ": nsteps must be >= 0");
  if (p->check_every < 1) throw ArgError(who + ": check_every must be >= 1");
  if (p->sample_every < 1) throw ArgError(who + ": sample_every must be >= 1");
  if (p->frame_every < 0) throw ArgError(who + ": frame_every must be >= 0 (0: no frames)");
  if (!positive(p->dt)) throw ArgError(who + ": dt must be a finite number > 0");
  if (!positive(p->ftm2v) || !positive(p->mvv2e)) throw ArgError(who + ": ftm2v and mvv2e must be finite numbers > 0");
  if (!std::isfinite(p->gamma) || p->gamma < 0.0) throw ArgError(who + ": gamma must be a finite number >= 0 (0: NVE)");
  if (read_kT && (!std::isfinite(p->kT) || p->kT < 0.0)) throw ArgError(who + ": kT must be a finite number >= 0");
  if ((frames != nullptr) != (p->frame_every > 0)) throw ArgError(who + ": frames must be NULL when frame_every is 0, and only then");
  if (natoms > 0 && (!v || !mass)) throw ArgError(who + ": v or mass is NULL");
  for (int i = 0; i < natoms; ++i) {
    if (!positive(mass[i])) throw ArgError(who + ": the mass of atom " + std::to_string(i) + " is not a finite number > 0");
    if (!std::isfinite(v[3 * i]) || !std::isfinite(v[3 * i + 1]) || !std::isfinite(v[3 * i + 2]))
      throw ArgError(who + ": the velocity of atom " + std::to_string(i) + " is not finite");
  }
  const size_t frame_rows = p->frame_every > 0 ? (size_t)(p->nsteps / p->frame_every) + 1 : 0;
  if ((double)frame_rows * (double)natoms * 3.0 * sizeof(double) > 1073741824.0)
    throw ArgError(who + ": the frames of this call would take more than 1 GiB on the device: call again with fewer steps and carry x, v and step0 over");
}

// MD (NVE, or Langevin by BAOAB) with the integrator's state on the device (algorithm and statuses: include/allegro_hip.h; kernels: neigh.hip).  The loop is that
// of ahip_relax_cell with a step count known in advance.  Nothing of the caller's is written before the last read-back has succeeded.
int ahip_md_cell(ahip_model *m, int natoms, double *x, double *v, const int *mtype, const double *mass, const double *cell, const int *pbc, double skin,
                 const int *fixed, const ahip_md_params *p, double *f, double *eatom, double *eng, double *virial, double *thermo, double *frames, int *evaluations,
                 int *rebuilds) {
  return guarded([&] {
    require_model(m);
    const std::string who = "ahip_md_cell";
    const std::vector<int> present = cell_check_args(m, who, natoms, x, mtype, cell, pbc, skin, f, eng);
    if (!(skin > 0.0)) throw ArgError(who + ": skin must be > 0 (the skin is what the atoms may move through before the list is rebuilt)");
    if (!p) throw ArgError(who + ": p is NULL (ahip_md_params_default fills one)");
    md_check_args(who, natoms, v, mass, p, frames, p->gamma > 0.0);
    const size_t thermo_rows = (size_t)(p->nsteps / p->sample_every) + 1, frame_rows = p->frame_every > 0 ? (size_t)(p->nsteps / p->frame_every) + 1 : 0;
    (void)cell_geometry(who.c_str(), cell, pbc, 1.0);      // a singular or non-finite cell is refused here, with the hold as it was
    *eng = 0;
    if (virial) for (int k = 0; k < 6; ++k) virial[k] = 0;
    if (evaluations) *evaluations = 0;
    if (rebuilds) *rebuilds = 0;
    if (natoms == 0) {                        // nothing to launch: the thermo rows of no atoms
      if (thermo) std::fill(thermo, thermo + 8 * thermo_rows, 0.0);
      return;
    }
    // Whatever fails from here on fails behind a launch and leaves nothing held.
    m->hold.serial = 0;
    AHIP_CHECK(hipSetDevice(m->device));
    hipStream_t s = nullptr;
    const double rc = *std::max_element(m->rcut_model_host.begin(), m->rcut_model_host.end()) + skin;
    MdPar par{};
    par.dt = p->dt; par.hdtf = 0.5 * p->dt * p->ftm2v; par.gamma = p->gamma; par.kT = p->gamma > 0.0 ? p->kT : 0.0; par.mvv2e = p->mvv2e; par.skin = skin;
    par.c1 = std::exp(-p->gamma * p->dt); par.c2 = std::sqrt(1.0 - par.c1 * par.c1);
    par.seed = p->seed; par.step0 = p->step0;
    par.nsteps = p->nsteps; par.sample_every = p->sample_every; par.frame_every = p->frame_every;
    int n = 0, nev = 0, nreb = 0, ng = 0;
    md_begin(*m, natoms, x, v, mass, fixed, thermo_rows, frame_rows, s);
    // rows, list and hold from the positions on the device (those of configuration n), then their forces
    const auto rebuild = [&] {
      ng = cell_rows(m, who, present, natoms, m->q_x[n & 1].as<double>(), true, mtype, cell, pbc, skin);
      cell_hold_take(*m, natoms, ng, cell, pbc, skin, rc, s);
      relax_rows_fresh(*m, natoms, s);
      nev += cell_evaluate_dev(m, who, natoms, ng, s);
      ++nreb;
    };
    rebuild();
    bool may_repeat = true;                   // NONFINITE or the alarm: once, under fused_arith=auto, the frozen configuration is evaluated again on the float32 instance
    for (;;) {
      const int chunk = std::min(p->check_every, p->nsteps - n);
      for (int k = 0; k < chunk; ++k) {       // no wait in here
        md_step(*m, (n + k) & 1, par, true, s);
        cell_evaluate_enqueue(m, natoms, ng, s);
        ++nev;
      }
      if (n + chunk == p->nsteps) md_step(*m, p->nsteps & 1, par, false, s);      // the last configuration is only checked and sampled: no evaluation behind it
      const MdState st = md_read(*m, s);
      n = st.n;
      if (const int bad = inactive_take(*m)) throw ArgError(who + ": " + inactive_message(*m, bad, "this evaluation") + " (nothing was written to x, v or f)");
      if (alarm_take(*m) || st.status == MD_NONFINITE) {
        if (!(arith_may_degrade(*m) && may_repeat && m->last_path.find("f16x2") != std::string::npos))      // (no other arithmetic has a float32 instance to fall back to)
          throw StateError(who + ": a force, the energy, the kinetic energy or a displacement was not finite after " + std::to_string(n) + " steps (coincident atoms, an input "
                           "that was not finite, a time step too large, or an activation left float16's range): the forces of this evaluation are invalid and nothing was "
                           "written to x, v or f" + (arith_effective(m->arith.opt) == ArithOpt::F16x2 ? "; set option fused_arith=f32 (or auto) for this model" : ""));
        may_repeat = false;
        arith_degrade(*m, "an MD run met a non-finite force or the float16-range alarm; the configuration of its last valid step was evaluated again");
        if (st.status != MD_NEED_REBUILD) {
          nev += cell_evaluate_dev(m, who, natoms, ng, s);
          md_resume(*m, s);
          continue;
        }
      }
      if (st.status == MD_DONE) break;
      if (st.status == MD_NEED_REBUILD) {
        rebuild();
        md_resume(*m, s);
      }
    }
    AHIP_CHECK(hipStreamSynchronize(s));
    AHIP_CHECK(hipGetLastError());
    copy_d2h(x, m->q_x[n & 1].p, (size_t)natoms * 3 * sizeof(double));
    copy_d2h(v, m->q_vnow.p, (size_t)natoms * 3 * sizeof(double));
    if (thermo) copy_d2h(thermo, m->q_thermo.p, thermo_rows * 8 * sizeof(double));
    if (frames) copy_d2h(frames, m->q_frames.p, frame_rows * (size_t)natoms * 3 * sizeof(double));
    cell_download(m, natoms, f, eatom, eng, virial);
    if (evaluations) *evaluations = nev;
    if (rebuilds) *rebuilds = nreb;
    m->hold.mtype.assign(mtype, mtype + natoms);
    m->hold.serial = m->list_serial;
  });
}

int ahip_debug_md_noise(unsigned long long seed, unsigned long long step, int n, double *out) {
  return guarded([&] {
    if (n < 0 || (n > 0 && !out)) throw ArgError("ahip_debug_md_noise: bad argument");
    if (n == 0) return;
    DevBuf d;
    d.reserve((size_t)n * 3 * sizeof(double));
    try {
      md_noise(seed, step, n, d.as<double>(), nullptr);
      AHIP_CHECK(hipStreamSynchronize(nullptr));
      copy_d2h(out, d.p, (size_t)n * 3 * sizeof(double));
    } catch (...) { d.release(); throw; }
    d.release();
  });
}

int ahip_npt_params_default(ahip_npt_params *p) {
  return guarded([&] {
    if (!p) throw ArgError("ahip_npt_params_default: p is NULL");
    *p = ahip_npt_params{ahip_md_params{0, 4, 1, 0, 0.001, 1.0 / 1.0364269e-4, 1.0364269e-4, 0.0, 0.0, 0ull, 0ull}, 0.0, 1.6, 1.0};
  });
}

// MD at constant pressure with the integrator's and the barostat's state on the device (algorithm and statuses: include/allegro_hip.h; kernels: neigh.hip).  The
// loop is that of ahip_md_cell; the cell of a rebuild is the one the state block holds.  Nothing of the caller's is written before the last read-back has succeeded.
int ahip_npt_cell(ahip_model *m, int natoms, double *x, double *v, const int *mtype, const double *mass, const double *cell, const int *pbc, double skin,
                  const int *fixed, const ahip_npt_params *p, double *cell_out, double *f, double *eatom, double *eng, double *virial, double *thermo, double *frames,
                  double *frame_cells, int *evaluations, int *rebuilds) {
  return guarded([&] {
    require_model(m);
    const std::string who = "ahip_npt_cell";
    const std::vector<int> present = cell_check_args(m, who, natoms, x, mtype, cell, pbc, skin, f, eng);
    if (!(skin > 0.0)) throw ArgError(who + ": skin must be > 0 (the skin is what the atoms and the cell may move through before the list is rebuilt)");
    if (!p) throw ArgError(who + ": p is NULL (ahip_npt_params_default fills one)");
    if (natoms == 0) throw ArgError(who + ": natoms is 0 (no atoms, no pressure)");
    if (!cell_out) throw ArgError(who + ": cell_out is NULL");
    if (!(pbc[0] && pbc[1] && pbc[2])) throw ArgError(who + ": all three axes must be periodic (the rescaling is isotropic)");
    md_check_args(who, natoms, v, mass, &p->md, frames, true);
    if (frame_cells && p->md.frame_every == 0) throw ArgError(who + ": frame_cells must be NULL when frame_every is 0");
    if (!std::isfinite(p->pressure)) throw ArgError(who + ": pressure must be finite");
    if (!std::isfinite(p->compressibility) || !(p->compressibility > 0.0)) throw ArgError(who + ": compressibility must be a finite number > 0");
    if (!std::isfinite(p->tau_p) || !(p->tau_p > 0.0)) throw ArgError(who + ": tau_p must be a finite number > 0");
    const ahip_md_params &q = p->md;
    const size_t thermo_rows = (size_t)(q.nsteps / q.sample_every) + 1, frame_rows = q.frame_every > 0 ? (size_t)(q.nsteps / q.frame_every) + 1 : 0;
    (void)cell_geometry(who.c_str(), cell, pbc, 1.0);      // a singular or non-finite cell is refused here, with the hold as it was
    *eng = 0;
    if (virial) for (int k = 0; k < 6; ++k) virial[k] = 0;
    if (evaluations) *evaluations = 0;
    if (rebuilds) *rebuilds = 0;
    // Whatever fails from here on fails behind a launch and leaves nothing held.
    m->hold.serial = 0;
    AHIP_CHECK(hipSetDevice(m->device));
    hipStream_t s = nullptr;
    const double rc = *std::max_element(m->rcut_model_host.begin(), m->rcut_model_host.end()) + skin;
    NptPar par{};
    par.md.dt = q.dt; par.md.hdtf = 0.5 * q.dt * q.ftm2v; par.md.gamma = q.gamma; par.md.kT = q.kT; par.md.mvv2e = q.mvv2e; par.md.skin = skin;
    par.md.c1 = std::exp(-q.gamma * q.dt); par.md.c2 = std::sqrt(1.0 - par.md.c1 * par.md.c1);
    par.md.seed = q.seed; par.md.step0 = q.step0;
    par.md.nsteps = q.nsteps; par.md.sample_every = q.sample_every; par.md.frame_every = q.frame_every;
    par.p0 = p->pressure; par.beta_over_tau = p->compressibility / p->tau_p;
    par.noise = std::sqrt(2.0 * q.kT * p->compressibility * q.dt / p->tau_p);
    int n = 0, nev = 0, nreb = 0, ng = 0;
    npt_begin(*m, natoms, x, v, mass, fixed, cell, thermo_rows, frame_rows, s);
    NptState st = npt_read(*m, s);
    // rows, list and hold from the positions on the device (those of configuration n) in the cell of the state block, then their forces
    const auto rebuild = [&] {
      ng = cell_rows(m, who, present, natoms, m->q_x[n & 1].as<double>(), true, mtype, st.geom.h, pbc, skin);
      cell_hold_take(*m, natoms, ng, st.geom.h, pbc, skin, rc, s);
      relax_rows_fresh(*m, natoms, s);
      nev += cell_evaluate_dev(m, who, natoms, ng, s);
      npt_held(*m, st, s);
      ++nreb;
    };
    rebuild();
    bool may_repeat = true;                   // NONFINITE or the alarm: once, under fused_arith=auto, the frozen configuration is evaluated again on the float32 instance
    for (;;) {
      const int chunk = std::min(q.check_every, q.nsteps - n);
      for (int k = 0; k < chunk; ++k) {       // no wait in here
        npt_step(*m, (n + k) & 1, par, true, s);
        cell_evaluate_enqueue(m, natoms, ng, s);
        ++nev;
      }
      if (n + chunk == q.nsteps) npt_step(*m, q.nsteps & 1, par, false, s);      // the last configuration is only checked and sampled: no evaluation behind it
      st = npt_read(*m, s);
      n = st.n;
      if (const int bad = inactive_take(*m)) throw ArgError(who + ": " + inactive_message(*m, bad, "this evaluation") + " (nothing was written to x, v, cell_out or f)");
      if (alarm_take(*m) || st.status == MD_NONFINITE) {
        if (!(arith_may_degrade(*m) && may_repeat && m->last_path.find("f16x2") != std::string::npos))      // (no other arithmetic has a float32 instance to fall back to)
          throw StateError(who + ": a force, the energy, the kinetic energy, the pressure, a displacement or the cell was not finite after " + std::to_string(n) +
                           " steps (coincident atoms, an input that was not finite, a time step too large, a tau_p far too small, or an activation left float16's "
                           "range): the forces of this evaluation are invalid and nothing was written to x, v, cell_out or f" +
                           (arith_effective(m->arith.opt) == ArithOpt::F16x2 ? "; set option fused_arith=f32 (or auto) for this model" : ""));
        may_repeat = false;
        arith_degrade(*m, "an MD run met a non-finite force or the float16-range alarm; the configuration of its last valid step was evaluated again");
        if (st.status != MD_NEED_REBUILD) {
          nev += cell_evaluate_dev(m, who, natoms, ng, s);
          npt_resume(*m, s);
          continue;
        }
      }
      if (st.status == MD_DONE) break;
      if (st.status == MD_NEED_REBUILD) rebuild();
    }
    AHIP_CHECK(hipStreamSynchronize(s));
    AHIP_CHECK(hipGetLastError());
    copy_d2h(x, m->q_x[n & 1].p, (size_t)natoms * 3 * sizeof(double));
    copy_d2h(v, m->q_vnow.p, (size_t)natoms * 3 * sizeof(double));
    if (thermo) copy_d2h(thermo, m->q_nthermo.p, thermo_rows * 10 * sizeof(double));
    if (frames) copy_d2h(frames, m->q_frames.p, frame_rows * (size_t)natoms * 3 * sizeof(double));
    if (frame_cells) copy_d2h(frame_cells, m->q_fcells.p, frame_rows * 9 * sizeof(double));
    cell_download(m, natoms, f, eatom, eng, virial);
    std::copy(st.geom.h, st.geom.h + 9, cell_out);
    if (evaluations) *evaluations = nev;
    if (rebuilds) *rebuilds = nreb;
    m->hold.mtype.assign(mtype, mtype + natoms);
    m->hold.serial = m->list_serial;
  });
}

int ahip_debug_npt_noise(unsigned long long seed, unsigned long long step, double *out) {
  return guarded([&] {
    if (!out) throw ArgError("ahip_debug_npt_noise: out is NULL");
    DevBuf d;
    d.reserve(sizeof(double));
    try {
      npt_noise(seed, step, d.as<double>(), nullptr);
      AHIP_CHECK(hipStreamSynchronize(nullptr));
      copy_d2h(out, d.p, sizeof(double));
    } catch (...) { d.release(); throw; }
    d.release();
  });
}

int ahip_last_cell_rows(ahip_model *m, int *nrows, long long *row_atom) {
  return guarded([&] {
    require_model(m);
    if (!nrows) throw ArgError("ahip_last_cell_rows: nrows is NULL");
    if (m->cell_natoms < 0) throw StateError("ahip_last_cell_rows called before ahip_compute_cell (or after an ahip_compute_cells that failed)");
    *nrows = m->cell_natoms + (int)m->cell_src_host.size();
    if (!row_atom) return;
    for (int i = 0; i < m->cell_natoms; ++i) row_atom[i] = i;
    std::copy(m->cell_src_host.begin(), m->cell_src_host.end(), row_atom + m->cell_natoms);
  });
}

int ahip_compute_cells(ahip_model *m, int nstruct, const int *first, const double *x, const int *mtype, const double *cells, const int *pbc, double skin,
                       double *f, double *eatom, double *eng, double *virial) {
  return guarded([&] {
    require_model(m);
    // ---- everything that can be refused is refused here: no launch before, nothing written before
    if (nstruct < 0 || (nstruct > 0 && (!first || !cells || !pbc || !eng))) throw ArgError("ahip_compute_cells: bad argument");
    if (!(skin >= 0.0) || !std::isfinite(skin)) throw ArgError("ahip_compute_cells: skin must be a finite number >= 0");
    if (nstruct > 0 && first[0] != 0) throw ArgError("ahip_compute_cells: first[0] must be 0");
    for (int s = 0; s < nstruct; ++s)
      if (first[s + 1] < first[s])
        throw ArgError("ahip_compute_cells: first is not non-decreasing: structure " + std::to_string(s) + " would have " + std::to_string(first[s + 1] - first[s]) + " atoms");
    const int natoms = nstruct > 0 ? first[nstruct] : 0;
    if (natoms > 0 && (!x || !mtype || !f)) throw ArgError("ahip_compute_cells: bad argument");
    const int T = m->hm.num_types;
    std::vector<int> sidx((size_t)natoms), present;
    std::vector<char> seen((size_t)T, 0);
    for (int s = 0; s < nstruct; ++s)
      for (int i = first[s]; i < first[s + 1]; ++i) {
        if (mtype[i] < 0 || mtype[i] >= T)
          throw ArgError("ahip_compute_cells: structure " + std::to_string(s) + ", atom " + std::to_string(i - first[s]) + " has model type " + std::to_string(mtype[i]) +
                         ", outside the model's " + std::to_string(T) + " types");
        for (int d = 0; d < 3; ++d)
          if (!std::isfinite(x[3 * (size_t)i + d])) throw ArgError("ahip_compute_cells: structure " + std::to_string(s) + ", atom " + std::to_string(i - first[s]) + ": a position is not finite");
        seen[(size_t)mtype[i]] = 1;
        sidx[(size_t)i] = s;
      }
    for (int t = 0; t < T; ++t) if (seen[(size_t)t]) present.push_back(t);       // the union of the types present: the active set of a model of more than 16 types
    const double rc = *std::max_element(m->rcut_model_host.begin(), m->rcut_model_host.end()) + skin;
    std::vector<unsigned char> table;
    double lo[3], hi[3];
    const size_t entry = cells_plan(nstruct, first, x, cells, pbc, rc, table, lo, hi);
    // ---- accepted
    for (int s = 0; s < nstruct; ++s) eng[s] = 0;
    if (virial) for (size_t k = 0; k < 6 * (size_t)nstruct; ++k) virial[k] = 0;
    // what the accessors report (ahip_last_cell_rows, ahip_last_cells_ghosts) is set when the call has succeeded; from here to there they have nothing to report,
    // because the row buffers are being overwritten
    const int guess = natoms == m->cell_natoms ? m->cell_nghost_last + m->cell_nghost_last / 8 : 0;
    m->cell_natoms = -1; m->cells_nstruct = -1;
    m->cell_src_host.clear();
    if (natoms == 0) {                        // a batch without atoms: nothing is launched; the neighbor list and the edges of an earlier evaluation stay as they are
      m->cell_natoms = 0; m->cell_nghost_last = 0;
      m->cells_nstruct = nstruct; m->cells_nghost_host.assign((size_t)nstruct, 0);
      return;
    }
    m->hold.serial = 0;                       // the rows of a list held by ahip_compute_cell_reuse are overwritten from here on
    AHIP_CHECK(hipSetDevice(m->device));
    hipStream_t s = nullptr;
    // ONE upload: positions | structure table | model types | atom -> structure (packed on the host first: a second pass over the input, O(atoms), instead of
    // four staged copies with a synchronisation each)
    const size_t o_tab = (size_t)natoms * 3 * sizeof(double), o_mt = o_tab + table.size(), o_sidx = o_mt + (size_t)natoms * sizeof(int),
                 n_in = o_sidx + (size_t)natoms * sizeof(int);
    if (entry % 8 != 0) throw StateError("ahip_compute_cells: structure table entries are not 8-byte multiples");      // (the int arrays follow the table)
    std::vector<unsigned char> in(n_in);
    std::memcpy(in.data(), x, o_tab);
    std::memcpy(in.data() + o_tab, table.data(), table.size());
    std::memcpy(in.data() + o_mt, mtype, (size_t)natoms * sizeof(int));
    std::memcpy(in.data() + o_sidx, sidx.data(), (size_t)natoms * sizeof(int));
    m->c_in.reserve(n_in);
    copy_h2d(m->c_in.p, in.data(), n_in);
    const char *base = m->c_in.as<char>();
    const double *x_in = (const double *)base;
    const void *tab = base + o_tab;
    const int *mt_in = (const int *)(base + o_mt), *sidx_dev = (const int *)(base + o_sidx);
    // wrap, count, scan (one read-back: the ghost total), fill.  The rows are the atoms of the batch, then its ghosts; the first guess of their number is the
    // last call's, and a grown buffer loses its content, so the wrap runs again behind it (the counts depend on the wrapped positions alone)
    auto room = [&](size_t ghosts) {
      m->c_x.reserve(((size_t)natoms + ghosts) * 3 * sizeof(double));
      m->c_mtype.reserve(((size_t)natoms + ghosts) * sizeof(int));
      cells_wrap(natoms, x_in, mt_in, sidx_dev, tab, m->c_x.as<double>(), m->c_mtype.as<int>(), s);
    };
    room((size_t)guess);
    const int ng = cells_count(*m, natoms, m->c_x.as<double>(), sidx_dev, tab, s);
    if (ng > guess) room((size_t)ng);
    const int nall = natoms + ng;             // (cells_plan has bounded atoms + images by 2^31 - 1 for any wrapped position)
    m->c_src.reserve(std::max<size_t>((size_t)ng, 1) * sizeof(long long));
    m->c_shift.reserve(std::max<size_t>((size_t)ng, 1) * 3 * sizeof(double));
    m->c_xp.reserve((size_t)nall * 3 * sizeof(double));
    cells_fill(*m, natoms, ng, m->c_x.as<double>(), m->c_mtype.as<int>(), sidx_dev, tab, m->c_x.as<double>() + 3 * (size_t)natoms, m->c_mtype.as<int>() + natoms,
               m->c_src.as<long long>(), m->c_shift.as<double>(), s);
    cells_place(natoms, nall, m->c_x.as<double>(), sidx_dev, m->c_src.as<long long>(), tab, m->c_xp.as<double>(), s);
    m->active_mapped = present;               // (run_model: resolve_active)
    neigh_build(*m, natoms, nall, m->c_xp.as<double>(), lo, hi, rc, s);
    m->c_f.reserve((size_t)nall * 3 * sizeof(double));
    m->c_eatom.reserve((size_t)nall * sizeof(double));
    m->c_engvir.reserve(8 * sizeof(double));
    m->c_out.reserve((size_t)nstruct * 8 * sizeof(double));
    // (twice at most, as in ahip_compute_cell: under fused_arith=auto a float16-range alarm repeats the whole batch on the float32 instance)
    for (int attempt = 0;; ++attempt) {
      AHIP_CHECK(hipMemsetAsync(m->c_f.p, 0, (size_t)nall * 3 * sizeof(double), s));
      AHIP_CHECK(hipMemsetAsync(m->c_eatom.p, 0, (size_t)nall * sizeof(double), s));
      rethrow_code(ahip_compute_dev(m, natoms, ng, m->c_xp.as<double>(), m->c_mtype.as<int>(), nullptr, m->c_f.as<double>(), m->c_eatom.as<double>(),
                                    m->c_engvir.as<double>(), s));
      cells_reduce(*m, nstruct, natoms, tab, m->c_x.as<double>(), m->c_f.as<double>(), m->c_eatom.as<double>(), m->c_out.as<double>(), s);
      comm_scatter_local(ng, natoms, m->c_src.as<long long>(), m->c_f.as<double>(), s);      // ghost forces go home (newton on), behind the row sums
      AHIP_CHECK(hipGetLastError());
      AHIP_CHECK(hipStreamSynchronize(s));
      if (const int bad = inactive_take(*m)) throw ArgError("ahip_compute_cells: " + inactive_message(*m, bad, "this evaluation") + " (nothing was written to f)");
      if (alarm_take(*m)) {
        if (arith_may_degrade(*m) && attempt == 0) {
          arith_degrade(*m, "an activation left float16's range (non-finite edge gradient on the f16x2 arithmetic); the evaluation was repeated");
          continue;
        }
        throw StateError("fused_arith=f16x2: an edge gradient was not finite (an activation left float16's range, or the input was not finite): the forces of this "
                         "batch are invalid and were not written to f; set option fused_arith=f32 (or auto) for this model");
      }
      break;
    }
    std::vector<double> out((size_t)nstruct * 8);
    copy_d2h(out.data(), m->c_out.p, out.size() * sizeof(double));
    copy_d2h(f, m->c_f.p, (size_t)natoms * 3 * sizeof(double));
    if (eatom) copy_d2h(eatom, m->c_eatom.p, (size_t)natoms * sizeof(double));
    m->cell_src_host.resize((size_t)ng);
    if (ng > 0) copy_d2h(m->cell_src_host.data(), m->c_src.p, (size_t)ng * sizeof(long long));
    m->cell_natoms = natoms; m->cell_nghost_last = ng;
    m->cells_nstruct = nstruct; m->cells_nghost_host.assign((size_t)nstruct, 0);
    for (int k = 0; k < nstruct; ++k) {
      eng[k] = out[8 * (size_t)k];
      if (virial) for (int c = 0; c < 6; ++c) virial[6 * (size_t)k + c] = out[8 * (size_t)k + 1 + c];
      m->cells_nghost_host[(size_t)k] = (long long)out[8 * (size_t)k + 7];
    }
  });
}

int ahip_last_cells_ghosts(ahip_model *m, int *nstruct, long long *nghost) {
  return guarded([&] {
    require_model(m);
    if (!nstruct) throw ArgError("ahip_last_cells_ghosts: nstruct is NULL");
    if (m->cells_nstruct < 0) throw StateError("ahip_last_cells_ghosts called before ahip_compute_cells (or after one that failed)");
    *nstruct = m->cells_nstruct;
    if (nghost) std::copy(m->cells_nghost_host.begin(), m->cells_nghost_host.end(), nghost);
  });
}

int ahip_nve_first_dev(ahip_model *m, int nlocal, int nall, double *x_dev, double *v_dev, double *f_dev, const int *mtype_dev,
                       const double *mass_by_mtype, double dt, double ftm2v, void *stream) {
  return guarded([&] {
    require_model(m);
    if (nlocal < 0 || nall < nlocal || (nall > 0 && !f_dev) || (nlocal > 0 && (!x_dev || !v_dev || !mtype_dev || !mass_by_mtype)))
      throw ArgError("ahip_nve_first_dev: bad argument");
    AHIP_CHECK(hipSetDevice(m->device));
    nve_first_step(*m, nlocal, nall, x_dev, v_dev, f_dev, mtype_dev, mass_by_mtype, m->hm.num_types, dt, ftm2v, (hipStream_t)stream);
  });
}

int ahip_nve_dev(ahip_model *m, int mode, int n, double *x_dev, double *v_dev, const double *f_dev,
                 const int *mtype_dev, const double *mass_by_mtype, double dt, double ftm2v, void *stream) {
  return guarded([&] {
    require_model(m);
    if (n < 0 || (n > 0 && (!x_dev || !v_dev || !f_dev || !mtype_dev || !mass_by_mtype))) throw ArgError("ahip_nve_dev: bad argument");
    if (mode != 0 && mode != 1) throw ArgError("ahip_nve_dev: mode must be 0 or 1");
    AHIP_CHECK(hipSetDevice(m->device));
    nve_step(*m, mode, n, x_dev, v_dev, f_dev, mtype_dev, mass_by_mtype, m->hm.num_types, dt, ftm2v, (hipStream_t)stream);
  });
}

// ---- diagnostics of the device-wide primitives and the generic path's GEMM: host buffers in, host buffers out, no model ----
namespace {
struct DebugBufs {                    // device buffers of one diagnostic call
  std::vector<void *> p;
  void *get(size_t bytes) {
    void *q = nullptr;
    AHIP_CHECK(hipMalloc(&q, bytes ? bytes : 1));
    p.push_back(q);
    return q;
  }
  void *upload(const void *host, size_t bytes) {
    void *q = get(bytes);
    if (bytes) copy_h2d(q, host, bytes);
    return q;
  }
  ~DebugBufs() { for (void *q : p) (void)hipFree(q); }
};
struct DebugScratch {
  PrimScratch ps;
  ~DebugScratch() { ps.release(); }
};
}  // namespace

int ahip_debug_scan_i32(const int *in, int n, int warm_n, int *out) {
  return guarded([&] {
    if (n < 0 || warm_n < 0 || warm_n > n || !out || (n > 0 && !in)) throw ArgError("ahip_debug_scan_i32: bad argument");
    DebugBufs b;
    DebugScratch sc;
    int *din = (int *)b.upload(in, (size_t)n * sizeof(int));
    int *dout = (int *)b.get(((size_t)n + 1) * sizeof(int));
    if (warm_n > 0) AHIP_CHECK(prim_exclusive_scan_i32(sc.ps, din, dout, warm_n, nullptr));      // a small scan first: the next one re-grows the scratch
    AHIP_CHECK(prim_exclusive_scan_i32(sc.ps, din, dout, n, nullptr));
    AHIP_CHECK(hipStreamSynchronize(nullptr));
    copy_d2h(out, dout, ((size_t)n + 1) * sizeof(int));
  });
}

int ahip_debug_sum_columns_f64(const double *in, long long nrow, int ncol, double *out) {
  return guarded([&] {
    if (nrow < 0 || ncol < 1 || !out || (nrow > 0 && !in)) throw ArgError("ahip_debug_sum_columns_f64: bad argument");
    DebugBufs b;
    DebugScratch sc;
    double *din = (double *)b.upload(in, (size_t)nrow * ncol * sizeof(double));
    double *dout = (double *)b.get((size_t)ncol * sizeof(double));
    AHIP_CHECK(prim_sum_columns_f64(sc.ps, din, nrow, ncol, dout, nullptr));
    AHIP_CHECK(hipStreamSynchronize(nullptr));
    copy_d2h(out, dout, (size_t)ncol * sizeof(double));
  });
}

int ahip_debug_max_i32(const int *in, int n, int *out) {
  return guarded([&] {
    if (n < 0 || !out || (n > 0 && !in)) throw ArgError("ahip_debug_max_i32: bad argument");
    DebugBufs b;
    int *din = (int *)b.upload(in, (size_t)n * sizeof(int));
    int *dout = (int *)b.get(sizeof(int));
    AHIP_CHECK(prim_max_i32(din, n, dout, nullptr));
    AHIP_CHECK(hipStreamSynchronize(nullptr));
    copy_d2h(out, dout, sizeof(int));
  });
}

int ahip_debug_gemm_f32(long long E, int K, int N, const float *A, int lda, int a_off, const float *W, int ldw, int transB, float *C, int ldc,
                        int accumulate, float *silu_out, const float *dsilu_z) {
  return guarded([&] {
    if (E < 1 || K < 1 || N < 1 || !A || !W || !C || a_off < 0 || lda < K || ldw < (transB ? K : N) || ldc < N)
      throw ArgError("ahip_debug_gemm_f32: bad argument");
    DebugBufs b;
    const size_t nC = (size_t)E * ldc * sizeof(float);
    const float *dA = (const float *)b.upload(A, ((size_t)a_off + (size_t)(E - 1) * lda + K) * sizeof(float));
    const float *dW = (const float *)b.upload(W, ((size_t)((transB ? N : K) - 1) * ldw + (transB ? K : N)) * sizeof(float));
    float *dC = (float *)b.upload(C, nC);
    float *dS = silu_out ? (float *)b.upload(silu_out, nC) : nullptr;
    const float *dZ = dsilu_z ? (const float *)b.upload(dsilu_z, nC) : nullptr;
    if (!gemm_f32(nullptr, E, K, N, dA + a_off, lda, dW, ldw, transB != 0, dC, ldc, accumulate != 0, dS, dZ))
      throw UnsupportedError("ahip_debug_gemm_f32: this build has no MFMA GEMM");
    AHIP_CHECK(hipGetLastError());
    AHIP_CHECK(hipStreamSynchronize(nullptr));
    copy_d2h(C, dC, nC);
    if (silu_out) copy_d2h(silu_out, dS, nC);
  });
}

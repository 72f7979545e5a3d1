/* allegro_hip.h -- C-ABI of liballegro_hip.so: the MI355X-native `pair_style allegro` hot path.
 *
 * Drop-in boundary.  The reference pair style (mir-group/pair_allegro,
 * pair_nequip_allegro.{h,cpp}) does, per MPI rank:
 *
 *     coeff()      : torch::jit::load(model) + metadata            pair_nequip_allegro.cpp:174-330
 *     compute()    : preprocess() -> call() -> scatter             pair_nequip_allegro.cpp:333-407
 *
 * with preprocess()/call() living in libtorch.  This library replaces everything below
 * `Pair::coeff` / `Pair::compute`: the model file reader, the cutoff filter of the LAMMPS
 * (skin-inflated) full neighbor list, the Allegro model itself (hand-written HIP kernels,
 * analytic backward) and the force / energy / virial read-out.  A LAMMPS `Pair` subclass only
 * marshals pointers into these entry points (pair_allegro_amd/lammps/pair_allegro_hip.cpp;
 * binding recipe in INTEGRATION.md).
 *
 * Conventions: every function returns 0 on success, non-zero on failure; the message is then
 * available from ahip_last_error() (thread-local).  Nothing here throws, exits or prints
 * (except the explicit debug dump).  Plain pointers and sizes only, no torch / LAMMPS types.
 * Pointers are HOST pointers unless the function name ends in `_dev`.
 * There is NO CPU fallback: every entry point that computes needs a gfx950 device.
 */
#ifndef ALLEGRO_HIP_H
#define ALLEGRO_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ahip_model ahip_model;

#define AHIP_OK 0
#define AHIP_ERR_ARG 1      /* bad argument / deck error  (-> LAMMPS error->all)            */
#define AHIP_ERR_FILE 2     /* model file problems (reference throws std::runtime_error, :205) */
#define AHIP_ERR_DEVICE 3   /* HIP runtime failure / no GPU                                  */
#define AHIP_ERR_STATE 4    /* call order (compute before neigh_update, ...)                */
#define AHIP_ERR_UNSUPPORTED 5

/* Message of the last failure on this thread ("" if none). */
const char *ahip_last_error(void);

/* Number of visible HIP devices; replaces torch::cuda::is_available()/device_count()
 * (pair_nequip_allegro.cpp:92,102).  The caller maps node-local rank -> device index exactly
 * like pair_nequip_allegro.cpp:93-120 (modulo wrap-around only in debug mode). */
int ahip_device_count(int *count);

/* Load `*.nequip.pth` (TorchScript archive carrying the `allegro_hip.bin` section) or a bare
 * `*.ahip` blob and upload the weights to `device`.  Replaces torch::jit::load + freeze
 * (pair_nequip_allegro.cpp:214-232).  Any other extension -> AHIP_ERR_FILE, like :197-206. */
int ahip_model_load(const char *path, int device, ahip_model **out);
void ahip_model_free(ahip_model *m);

/* Model metadata = the five keys the reference reads from the archive
 * (pair_nequip_allegro.cpp:214-220; consumed :267-328).  Any out-pointer may be NULL.
 *   type_names: whitespace-separated, model-type order (:275-294)
 *   per_edge_type_cutoff: row-major [num_types][num_types] in MODEL type index, or NULL when the
 *                         model has a single r_max (:303-328)
 * Returned pointers live as long as the model. */
int ahip_model_meta(const ahip_model *m, double *r_max, int *num_types, const char **type_names,
                    const double **per_edge_type_cutoff, int *l_max, int *num_tensor_features,
                    int *num_scalar_features, int *num_layers, const char **model_dtype);

/* Options (string key/value):
 *   "path"      = "auto" | "fused" | "generic"   kernel family (auto: fused when the model shape
 *                                                 and the per-atom edge counts allow it).  Fused shapes: l_max 1 or 2, up to 64 tensor features, up to 64
 *                                                 scalars, read-out width up to 32, MLP width up to 64 on every fused kernel and arithmetic, 65..128 on the
 *                                                 kernels for up to 32 tensor features (zero-padded to 128: f16x2 arithmetic with the tabulated two-body
 *                                                 embedding, read-out depth 1); read-out width 33..64 on every fused kernel (zero-padded to 64: f16x2
 *                                                 arithmetic with the tabulated two-body embedding, MLP width up to 64, read-out depth 1; wider than 64:
 *                                                 the layer-at-a-time kernels); narrower models run zero-padded
 *   "precision" = "model" | "float64"            compute dtype; float64 is the debug/parity build
 *   "chunk_edges" = "<n>"                        max edges processed per pass (workspace bound)
 *   "reserve_wgs" = "<n>"                        half-CU workgroup slots the persistent fused kernels leave unoccupied, so that
 *                                                 kernels launched on OTHER streams (ghost exchange) can run beside them (default 0)
 *   "cutoff_compare" = "le" | "lt"               edge kept iff rsq <= cut^2 (default; pair_nequip_allegro.cpp:507) or rsq < cut^2
 *                                                 (the KOKKOS path of the reference, pair_nequip_allegro_kokkos.cpp:174)
 *   "fused_arith" = "auto" | "f32" | "f16x2" | "bf16x3" | "tf32eq"   arithmetic of the dense contractions of the fused kernels: f32-input MFMA (exact float32
 *                                                 fmaf chains); two float16 terms per operand, three f16-MFMA products (float32-equivalent inside float16's exponent
 *                                                 range; an evaluation that leaves it returns AHIP_ERR_STATE: host-pointer calls at once, _dev calls at the next
 *                                                 evaluation); three-term bf16 split (float32-equivalent; k_fused, i.e. l_max = 1 with up to 32 tensor features);
 *                                                 two-term bf16 split (TF32-class; k_fused).  auto = f16x2 unless the model file says allow_tf32 = 1 (pair_nequip_allegro.cpp:267-270), then tf32eq.
 *                                                 auto is never less robust than the reference's float32 (which only ever RELAXES precision, :267-270): a model the split
 *                                                 cannot carry (a weight beyond float16's range, a linear inside its subnormals), a first evaluation that disagrees with
 *                                                 the float32 instance by more than 1e-5 max|F|, or a float16-range alarm switch the model to the f32 instance for the
 *                                                 rest of its life -- host-pointer calls re-evaluate inside the same call, _dev calls report the invalid earlier
 *                                                 evaluation once (AHIP_ERR_STATE) and continue on f32.  ahip_arith_note says what was decided.  Only an explicit
 *                                                 "f16x2" keeps the hard errors.
 *   "fused_tb"  = "table" | "mlp"                two-body embedding of the fused kernels: tabulated cubic splines (default) or the MLP itself
 *   "edge_schedule" = "auto" | "static" | "dynamic"   unit schedule of the single-pass edge build (dynamic: safe beside other resident kernels)
 *   "tile_pack" = "auto" | "separate" | "fused"  tile packing of the fused kernels inside the edge build or as its own kernels
 *   "dense_centres" = "whole" | "split"          a list in which a few centres have more edges than a tile of the fused kernel holds (128 for l_max = 1 with up to 32
 *                                                 tensor features, 64 for every other fused shape) while a list row is longer than 128 entries: "whole" (default) evaluates the whole list on the
 *                                                 layer-at-a-time kernels; "split" keeps the fused kernel for the other centres and evaluates only those few
 *                                                 (at most one centre in eight, else as "whole") on the layer-at-a-time kernels.  ahip_last_heavy_centres
 *                                                 reports them.  The cost of the split route has not been measured.
 *   "wide_tile" = "64" | "auto"                  tile shape of the l_max = 2 kernel with up to 32 tensor features (k_fused_lx): "64" (default) keeps its 64-slot tiles, so a
 *                                                 centre with more than 64 edges is one of the few above ("heavy"); "auto" lets the list's largest degree pick a second
 *                                                 shape of 128 slots (8 waves) as the l_max = 1 kernel does, so centres with 65..128 edges stay on the fused kernel and only
 *                                                 centres above 128 are heavy (the one-in-eight rule of "dense_centres" counts against 128 as well).  The second shape exists
 *                                                 for MLP depth 2, MLP width up to 64 and read-out depth 1 on the f32 and f16x2 arithmetics; for every other model (64 tensor features,
 *                                                 l_max = 1, other depths, MLP width 65..128, read-out width 33..64) "auto" behaves as "64" and is not an error.  Measured on one MI355X, 108 000-atom
 *                                                 fcc box with 78 edges per centre, 3 layers, 32 tensor features (tools/wide_tile_cost.py): 79.5 ms per evaluation
 *                                                 with "auto" against 265 ms with "64" (every centre heavy), the latter equal to the release before the option.  Not
 *                                                 measured on other lists, which is why the default stays "64".
 *   "lx64_mlp_width" = "64" | "auto"             MLP width of the kernel for 33..64 tensor features (k_fused_lx2: l_max = 2, or l_max = 1 lifted): "64" (default) keeps it at MLP
 *                                                 width up to 64, so such a model with mlp_width 65..128 runs on the layer-at-a-time kernels; "auto" lets it run on the kernel's
 *                                                 width-128 instances, zero-padded to 128, under the rules of that width on the other kernels: f16x2 arithmetic, read-out
 *                                                 depth 1, read-out width up to 32, and here allow_tf32 = 0 (anything else: the layer-at-a-time kernels, as without the
 *                                                 option).  For every other model (MLP width up to 64, up to 32 tensor features) "auto" changes nothing.  Measured on one
 *                                                 box and one model shape only (41 472-atom water, model L with 64 tensor features: tools/mlp_width_cost.py --configs 5:24,
 *                                                 profiles/lx64_mlp_width_cost.txt), which is why the default stays "64".
 *   "env_backward" = "auto" | "centre" | "edge"  the transposed environment linear of k_fused's backward pass (l_max = 1 kernel, f16x2 arithmetic, 64-slot tiles): "auto"
 *                                                 (default) evaluates it once per centre atom on tiles of up to 3 centres (one wave of the tile runs it on the centre's reduced
 *                                                 gradient, every edge combines four vectors: DESIGN 4.2g) and per edge on tiles of 4..6 centres; "centre" is the same rule
 *                                                 (tiles of more than 3 centres have no per-centre form); "edge" evaluates it per edge on every tile, as every other
 *                                                 arithmetic, tile shape and kernel does.  The two forms differ in rounding order only.  For A/B runs and tests.
 *   "timing"    = "0" | "1"                      record per-stage HIP events (ahip_get_timings)
 * Unknown keys and values are errors (AHIP_ERR_ARG).
 */
int ahip_set_option(ahip_model *m, const char *key, const char *value);

/* Hand over the LAMMPS full neighbor list -- only on steps where LAMMPS rebuilt it.
 * Replaces the list walk of preprocess() (pair_nequip_allegro.cpp:469-480,489-496).
 *   inum      : number of centre atoms (== nlocal, asserted at :470)
 *   nall      : nlocal + nghost (size of x / f / type)
 *   ilist     : [inum] centre atom indices
 *   numneigh  : indexed by ATOM index i (LAMMPS convention), numneigh[i]
 *   firstneigh: indexed by atom index i, firstneigh[i][0..numneigh[i])
 *   neighmask : LAMMPS NEIGHMASK; every j is stored as (j & neighmask) (:496)
 */
int ahip_neigh_update(ahip_model *m, int inum, int nall, const int *ilist, const int *numneigh,
                      const int *const *firstneigh, int neighmask);

/* Same, from a flat CSR list: neighbours of centre ii are neigh[offsets[ii] .. offsets[ii+1]). */
int ahip_neigh_update_csr(ahip_model *m, int inum, int nall, const int *ilist,
                          const long long *offsets, const int *neigh, int neighmask);
/* Same, CSR arrays already on the device (int32 offsets [inum+1]); no copy is made of `neigh`
 * -- the caller keeps it alive until the next update.  Synchronises the device once (the longest row is measured here: it bounds
 * every centre's degree until the next hand-over, which is what lets ahip_compute_dev* run without any device -> host read-back).
 * The CSR arrays MUST NOT change between hand-overs: a row that has grown past the measured bound is detected (the edge build's overflow word is
 * inspected, without waiting, by the following calls and by every accessor) and reported as AHIP_ERR_STATE by a LATER call -- the forces of the
 * evaluation that met it are invalid. */
int ahip_neigh_update_dev(ahip_model *m, int inum, int nall, const int *ilist_dev,
                          const int *offsets_dev, const int *neigh_dev, long long nneigh_total);

/* Same, from the device-resident list of the LAMMPS KOKKOS package: a padded 2-D table d_neighbors(i, jj) addressed as
 * neighbors_dev[i * stride_atom + jj * stride_slot] (column-major on a GPU build: stride_atom = 1), numneigh_dev indexed by ATOM
 * index, ilist_dev [inum].  Replaces the per-step table walk of pair_nequip_allegro_kokkos.cpp:128-131,142-181 (there every
 * step; here once per list rebuild: the table is compacted on the device into the library's own CSR rows, nothing is kept of
 * the caller's arrays).  Synchronises `stream` (two 4-byte read-backs). */
int ahip_neigh_update_dev_table(ahip_model *m, int inum, int nall, const int *ilist_dev, const int *numneigh_dev,
                                const int *neighbors_dev, long long stride_atom, long long stride_slot, int neighmask,
                                void *stream);

/* LAMMPS types (1-based, device) -> model types (device) through the pair_coeff mapping `type_mapper` [ntypes] (host, -1 =
 * unmapped); what pair_nequip_allegro_kokkos.cpp:222-223 does every step.  Fails if an atom carries an unmapped type.
 * Synchronises `stream`; callers run it on list-rebuild steps (the type of an atom index cannot change in between). */
int ahip_map_types_dev(ahip_model *m, int n, const int *type_dev, int ntypes, const int *type_mapper, int *mtype_dev,
                       void *stream);

/* Active types: the model types a simulation can produce.  The reference maps every LAMMPS type to one model type by name
 * (pair_nequip_allegro.cpp:274-294) and evaluates a model of tens of types like any other, however few of them `pair_coeff * * file A B C`
 * names.  Here the fused kernels hold at most 16 types (4-bit packed edge types), but a type enters them only as a row of the first two-body
 * linear, as scale / shift and as a row and column of the cutoff matrix: a fused evaluation therefore runs on the model restricted to its
 * active types (compact slots in ascending model-type order), and a model qualifies when at most 16 of its types are ACTIVE, whatever their
 * total (up to 255; beyond that, as with more than 16 active types, the layer-at-a-time kernels run and option path=fused says why).
 * The layer-at-a-time kernels, ahip_model_meta and the registered outputs always see the model as loaded.
 *   Automatic rule (no model that the fused kernels already served changes its behaviour): a model of MORE than 16 types takes the set from the
 *   type mapping -- ahip_compute from its type_mapper argument (entries >= 0), device-resident callers from the mapper last given to
 *   ahip_map_types_dev.  A model of at most 16 types runs whole.
 *   ahip_set_active_types names the set explicitly for any model (n entries, duplicates allowed, any order; a value outside the model's types
 *   is AHIP_ERR_ARG); n = 0 returns to the automatic rule.  It takes effect at the next evaluation; a change of the set rebuilds the prepared
 *   weight streams and two-body tables there (once).  For a model of at most 16 types a subset shrinks the two-body table (0.5 MB per type
 *   pair), which may well help a 10-type model that runs on two types; nobody has measured it, so it is not the default.
 *   An atom whose type is not in the set makes that evaluation's forces invalid; every index stays in range.  It is reported as AHIP_ERR_ARG
 *   naming the model type: by ahip_compute in the same call, before f is touched; to a device-resident caller by its next evaluation or
 *   accessor (ahip_get_active_types, ahip_get_edges, ahip_get_timings), once the device has got that far.  Under the automatic rule it cannot
 *   happen through ahip_compute / ahip_map_types_dev, which refuse unmapped types themselves.
 *   ahip_get_active_types: the set the last evaluation ran with, ascending (model_types: room for num_types entries, or NULL for the count
 *   alone); *n = 0: no subset. */
int ahip_set_active_types(ahip_model *m, int n, const int *model_types);
int ahip_get_active_types(ahip_model *m, int *n, int *model_types);

/* One force evaluation = PairNequIPAllegro<false>::compute (pair_nequip_allegro.cpp:333-407).
 *   x            [nall][3] f64 positions, locals first then ghosts (atom->x)
 *   type         [nall] LAMMPS types, 1-based (atom->type)
 *   ntypes       atom->ntypes
 *   type_mapper  [ntypes] LAMMPS type-1 -> model type, -1 = unmapped (:274-294)
 *   cutoff_matrix[ntypes*ntypes] in LAMMPS type index (:303-328); edge kept iff rsq <= cut^2 (:507)
 *   f            [nall][3]  forces are ADDED (f[i] += ...) for locals AND ghosts (:370-377)
 *   eatom        [nall] or NULL; eatom[i] = E_i is written for the inum centre atoms (:378)
 *   eng          out: sum of E_i over centre atoms only (:379)
 *   virial       out or NULL: xx,yy,zz,xy,xz,yz, no sign change (:387-392)
 */
int ahip_compute(ahip_model *m, int nlocal, int nghost, const double *x, const int *type, int ntypes,
                 const int *type_mapper, const double *cutoff_matrix, double *f, double *eatom,
                 double *eng, double *virial);

/* Device-resident variant (the pattern of pair_nequip_allegro_kokkos.cpp:109-126,266-268,305-319):
 * x_dev/f_dev/eatom_dev are device pointers, mtype_dev holds MODEL types (already mapped),
 * cutoff_matrix_model is a HOST [num_types^2] matrix in model-type index (NULL = r_max).
 * Forces are accumulated into f_dev; eng_vir_dev receives 7 doubles {eng, xx,yy,zz,xy,xz,yz}.
 * Asynchronous on `stream` (a hipStream_t, NULL = default).  The reference's Kokkos path reads its edge total back in every step
 * (:203-206); here the counters of the edge build (edge total, largest degree, centres left to the layer-at-a-time kernels) travel to
 * page-locked memory behind the edge build and the host waits for them only when it needs a value: never on the l_max = 1 fused path with
 * list rows of at most 128 entries (the row length measured at ahip_neigh_update* bounds every degree; tile shape and tile count are
 * decided on the device), after the model kernel has been enqueued on the wide fused paths (number of centres with more than 64 edges),
 * before the model on the layer-at-a-time path, and in the getters (ahip_get_edges, ahip_last_max_degree, ahip_last_heavy_centres, ahip_last_tile_occupancy).
 * With outputs registered through ahip_output_register the call additionally keeps host copies of them
 * (pair_nequip_allegro_kokkos.cpp:342-344) and synchronises the stream. */
int ahip_compute_dev(ahip_model *m, int nlocal, int nghost, const double *x_dev, const int *mtype_dev,
                     const double *cutoff_matrix_model, double *f_dev, double *eatom_dev,
                     double *eng_vir_dev, void *stream);

/* Same evaluation restricted to the centre atoms ilist[centre_begin .. centre_end) of the installed list (their edges, their
 * energies; forces still go to every atom they touch).  eng_vir_dev receives this range's partial sums.  This is what lets a
 * caller overlap the ghost exchange with the force evaluation (SURVEY 8e "Overlap"): centres whose whole neighbourhood is
 * local are evaluated while ghost positions are in flight, the boundary centres afterwards
 * (the reference evaluates all centres in one libtorch call after the exchange: pair_nequip_allegro.cpp:333-407). */
int ahip_compute_dev_range(ahip_model *m, int centre_begin, int centre_end, int nlocal, int nghost, const double *x_dev,
                           const int *mtype_dev, const double *cutoff_matrix_model, double *f_dev, double *eatom_dev,
                           double *eng_vir_dev, void *stream);

/* Number of entries of the installed (skin-inflated) neighbor list: sum of numneigh over the centre atoms
 * (the walk of pair_nequip_allegro.cpp:489-496 visits exactly these). */
long long ahip_last_list_size(ahip_model *m);

/* `compute allegro` / `compute allegro/atom` support: named entries of the model's output dict kept from the last
 * ahip_compute call (reference: the pair style stashes `output.at(name)` for every name registered through
 * add_custom_output, pair_nequip_allegro.cpp:403-406,681-684; compute/compute_allegro.cpp:81,114,145 reads them).
 * Entries this model's graph returns: "atomic_energy" [nlocal+nghost] (ghosts carry only their per-type shift, as in the
 * TorchScript model), "forces" [nlocal+nghost][3] (this evaluation's forces, before they are added to f),
 * "virial" [3][3], "total_energy" [1] (sum of atomic_energy over locals AND ghosts, cf. compute/README.md), and this
 * library's own "atomic_virial" [nlocal+nghost][9], the per-atom virial for a heat current:
 *     W_j[a][b] = - sum over the edges e = (i -> j) with NEIGHBOUR j of r_e[a] * dE/dr_e[b],   r_e = x_j - x_i,  row-major a, b
 * not symmetrised; ghost rows belong to their owners (reverse-communicate them: `compute ID all allegro/atom atomic_virial 9 1`);
 * the symmetric part of the sum over all rows is "virial".  Only a registered "atomic_virial" allocates its [nall][9] device
 * buffer and selects the model kernels' instances that produce it.
 * ahip_output_register: unknown names are accepted here and fail at the next ahip_compute, like the reference's
 * `output.at(name)`.  ahip_output_get copies the flattened tensor (capacity in doubles; *count = its length; pass out = NULL
 * to query the length).  ahip_compute and ahip_compute_dev (not ahip_compute_dev_range). */
int ahip_output_register(ahip_model *m, const char *name);
int ahip_output_get(ahip_model *m, const char *name, double *out, long long capacity, long long *count);

/* Edge list of the last compute: the tensors the reference would have handed to the model
 * (edge_index i64 [2][E], pair_nequip_allegro.cpp:601-602) plus |r_ij|.  Pass NULL buffers to
 * query nedges only.  This is what the `_NEQUIP_LOG_LEVEL=DEBUG` dump prints (:562-565,625). */
int ahip_get_edges(ahip_model *m, long long *nedges, long long *edge_index, double *rij);

/* Print "Allegro edges: i j rij" ... "end Allegro edges" to stdout with 0-based tag-1 ids and
 * %.10g distances, the exact format of pair_nequip_allegro.cpp:564,625,632.  tag may be NULL
 * (then atom indices are printed). */
int ahip_debug_dump_edges(ahip_model *m, const int *tag);

/* Per-stage device timings (option timing=1; HIP events on the launch stream): for every stage the SUM of its durations (ms) over the calls
 * since the previous ahip_get_timings -- called after every compute it is that compute's timing; names is a ';'-separated list valid until
 * the next call.  Waits for the recorded stages to finish; the compute calls themselves never wait for their events.
 * ahip_get_timing_counts: the number of launches behind each of those sums (same order), valid until the next ahip_get_timings. */
int ahip_get_timings(ahip_model *m, const char **names, const double **ms, int *n);
int ahip_get_timing_counts(ahip_model *m, const double **counts, int *n);

/* Diagnostics: edge slots of the tiles of the last fused evaluation (tiles x slots per tile) and the number that held an edge (= edges of
 * that call); their ratio is the packing efficiency bench.py reports as slots_used / slots_total.  0 / 0 after a non-fused evaluation. */
int ahip_last_tile_occupancy(ahip_model *m, long long *slots_used, long long *slots_total);

/* The model file's fifth metadata key, `allow_tf32` ("0" / "1").  The reference hands it to libtorch
 * (pair_nequip_allegro.cpp:267-270: at::globalContext().setAllowTF32CuBLAS / CuDNN): 1 = the model's author permits TF32-class
 * matrix arithmetic.  Here: with 1 (and option fused_arith=auto, the default) the fused model-S kernel runs its linears on the bf16
 * matrix cores with a two-term split (ahip_last_path reports "fused_tf32eq"); with 0 every path is float32-exact, float32-equivalent ("fused_f16x2", the default of the fused kernels) or better. */
int ahip_model_allow_tf32(const ahip_model *m, int *allow);

/* Kernel family and arithmetic used by the last compute: "generic_f32" | "generic_f64" | "fused_f16x2" | "fused_f32" | "fused_bf16x3" | "fused_tf32eq" ("" before). */
const char *ahip_last_path(ahip_model *m);
/* What fused_arith=auto decided for this model and why, one line ("" before the first evaluation): "fused_arith=auto: f16x2 kept: first evaluation within
 * ... of the float32 instance" or "fused_arith=auto: float32 instance (f32-input MFMA) selected: <reason>". */
const char *ahip_arith_note(const ahip_model *m);
/* Largest number of edges of any centre atom in the last compute. */
int ahip_last_max_degree(ahip_model *m);
/* Centres, and their edges, that the last compute evaluated on the layer-at-a-time kernels BESIDE a fused kernel: the centres with more than 64 edges of the
 * l_max = 2 kernels, and with option dense_centres=split those of every fused kernel behind list rows of more than 128 entries.  0 / 0 when there were none
 * or the path was not a fused one.  Waits for the edge build's counters when they are still in flight, like ahip_last_max_degree. */
int ahip_last_heavy_centres(ahip_model *m, int *ncentres, long long *nedges);

/* Diagnostic: single-wave self-test of the fused path's register-chain MFMA primitive,
 * out[32][N] = in[32][K] @ W[K][N] (W row-major f64, in/out f32 host buffers).
 * With AHIP_DEBUG_SPLIT=mix|ref in the environment and N == K: the f16x2 operand split alone, in its mixed-fma or its reference form; out receives
 * 32 K words: the 16 K packed hi terms of the pairs (in[2 i], in[2 i + 1]), then their 16 K packed lo' terms.  W is not read. */
int ahip_debug_fused_linear(int K, int N, const double *W, const float *in, float *out);

/* Diagnostics of the device-wide primitives (csrc/prims.hip) and of the layer-at-a-time path's float32 GEMM (csrc/gemm.hip): host buffers in, host
 * buffers out, no model.  Each call owns its scratch and synchronises the device.
 *   ahip_debug_scan_i32        : out[0..n] = exclusive prefix sum of in[0..n), out[n] = total.  warm_n > 0: in[0..warm_n) is scanned first on the same
 *                                scratch and the result discarded, so that the scan of n re-grows the scratch.
 *   ahip_debug_sum_columns_f64 : out[c] = sum_r in[r * ncol + c]; 1 <= ncol <= 8, anything else is an error before any launch.
 *   ahip_debug_max_i32         : out[0] = max(0, max(in[0..n))).
 *   ahip_debug_gemm_f32        : C[e][n] (+)= sum_k A'[e][k] * (transB ? W[n][k] : W[k][n]),  A' = A + a_off with row stride lda (A is uploaded whole,
 *                                [a_off + (E - 1) lda + K] floats, so a_off makes views that are not 16-byte aligned); C [E][ldc] is uploaded first
 *                                (accumulate, and the columns beyond N stay as they were).  silu_out / dsilu_z (either may be NULL) are the fused epilogues
 *                                of the model's dense layers, [E][ldc] like C: C *= silu'(dsilu_z), then silu_out = silu(C); silu_out is uploaded first, too.
 *                                AHIP_ERR_UNSUPPORTED in a build without the MFMA kernel. */
int ahip_debug_scan_i32(const int *in, int n, int warm_n, int *out);
int ahip_debug_sum_columns_f64(const double *in, long long nrow, int ncol, double *out);
int ahip_debug_max_i32(const int *in, int n, int *out);
int ahip_debug_gemm_f32(long long E, int K, int N, const float *A, int lda, int a_off, const float *W, int ldw, int transB, float *C, int ldc,
                        int accumulate, float *silu_out, const float *dsilu_z);

/* Diagnostic (environment AHIP_FUSED_DBG=1): per-edge {g[3], dE/dd, dE/dfc, dE/dY1..3} of the last fused
 * compute, [nedges][8] floats, edge order = ahip_get_edges. */
int ahip_debug_fused_edges(ahip_model *m, float *out, long long nedges);

/* ---- mini-MD helpers used by the stand-alone driver / bench (device-resident) ------------- */

/* Build a full neighbor list with cutoff rc_list (= r_max + skin) for nlocal centre atoms among
 * nall atoms (ghost images already materialised), binned cell list on the GPU.  The result is
 * owned by the model and installed as its current list (as if ahip_neigh_update_dev was called). */
int ahip_build_neighbors_dev(ahip_model *m, int nlocal, int nall, const double *x_dev,
                             const double *lo, const double *hi, double rc_list, void *stream);

/* Re-neighboring criterion of a stand-alone driver (LAMMPS' `neigh_modify check yes` test, Neighbor::check_distance, evaluated
 * one step ahead): flag_dev[0] = 1 iff max_i |x_i - xhold_i| + 2 dt max_i |v_i| > half_skin over the n local atoms.  Two launches on
 * `stream`, no host synchronisation (the caller all-reduces the flag and reads it a step later). */
int ahip_reneighbor_flag_dev(ahip_model *m, int n, const double *x_dev, const double *xhold_dev, const double *v_dev, double dt,
                             double half_skin, int *flag_dev, void *stream);

/* Ghost atoms of ONE rank that owns the whole periodic box (the stand-alone driver's `borders` step at a re-neighboring; LAMMPS' Comm::borders on a
 * 1 x 1 x 1 grid): every periodic image of an owned atom that lies inside the halo of thickness rc around [lo, hi) -- shift +box_d allowed where
 * x_d < lo_d + rc, -box_d where x_d >= hi_d - rc, every combination but (0, 0, 0).  Writes, per ghost, its position, model type, the index of the
 * owned atom it images (int64) and the shift (what ahip_comm_set_plan_local takes); *nghost is the number of images, which may exceed `capacity`
 * (then only the first `capacity` were written: call again with larger arrays).  Needs box_d >= rc.  Synchronises `stream` (one 4-byte read-back). */
int ahip_borders_local_dev(ahip_model *m, int nlocal, const double *x_dev, const int *mtype_dev, const double *lo, const double *hi,
                           const double *box, double rc, int capacity, double *xg_dev, int *mtg_dev, long long *src_dev, double *shift_dev,
                           int *nghost, void *stream);

/* ---- any periodic cell, one rank: triclinic cells, cells thinner than the cutoff, open axes ----
 * Conventions: `cell` is a HOST row-major double[9] whose rows are the lattice vectors (any orientation, not only LAMMPS' lower-triangular form), `pbc` a HOST
 * int[3] (non-zero = periodic axis), s = x . cell^-1 the fractional coordinates, h_d the height of the cell along d and m_d = rc / h_d.  A singular cell or one
 * with a non-finite entry is AHIP_ERR_ARG before any launch. */

/* LAMMPS' Domain::remap at a re-neighboring, for a general cell: adds to every position the integer lattice combination that brings s_d into [0, 1) on every
 * periodic axis; the fractional components of open axes are left alone, and an atom already inside comes back bit for bit.  One launch on `stream`, no host
 * synchronisation. */
int ahip_wrap_cell_dev(ahip_model *m, int n, double *x_dev, const double *cell, const int *pbc, void *stream);

/* Ghost atoms of ONE rank that owns the whole cell -- LAMMPS' Comm::borders on a 1 x 1 x 1 grid of a triclinic or thin box, where ahip_borders_local_dev needs an
 * orthogonal box with box_d >= rc.  For wrapped positions the image n = (n1, n2, n3) != 0 of atom i is a ghost iff for every d: n_d == 0 on an open axis,
 * -m_d <= s_id + n_d < 1 + m_d on a periodic one (LAMMPS' slab criterion in fractional coordinates: every image within rc of an atom of the cell satisfies it, and
 * on an orthogonal box with box_d >= rc it is the rule of ahip_borders_local_dev).  Any number of images per direction.  Writes, per ghost, its position
 * x_i + n . cell, the model type of i, the index i (int64) and the shift n . cell (what ahip_comm_set_plan_local takes), ordered by ascending source atom and, within
 * an atom, by (n1, n2, n3) ascending with n3 fastest.  Output contract of ahip_borders_local_dev: *nghost is the number of images and may exceed `capacity` (then
 * only the first `capacity` rows were written: call again with larger arrays).  nlocal x prod_d (2 ceil(m_d) + 1) must fit 32 bits (AHIP_ERR_ARG before any
 * launch otherwise).  Synchronises `stream` (one 4-byte read-back). */
int ahip_borders_cell_dev(ahip_model *m, int nlocal, const double *x_dev, const int *mtype_dev, const double *cell, const int *pbc, double rc, int capacity,
                          double *xg_dev, int *mtg_dev, long long *src_dev, double *shift_dev, int *nghost, void *stream);

/* One-call evaluation without LAMMPS -- "cell, positions, species in; energy, forces, virial out" -- i.e. everything LAMMPS does for the reference around
 * PairNequIPAllegro::compute on one rank (Domain::remap, Comm::borders, the full neighbor list, the reverse communication of newton_pair on,
 * pair_nequip_allegro.cpp:143-149,366-377).  HOST pointers.
 *   x      [natoms][3] positions, wrapped or not            mtype  [natoms] MODEL types, 0-based (a value outside the model's types: AHIP_ERR_ARG)
 *   skin   >= 0: only inflates the ghost shell and the list (rc = largest model cutoff + skin); the cutoffs are the model's own (r_max or its per-edge-type matrix)
 *   f      [natoms][3] and eatom [natoms] (or NULL) are WRITTEN, not accumulated, in the caller's atom order (ghost forces already added to their sources)
 *   eng    energy;  virial [6] or NULL: xx,yy,zz,xy,xz,yz in LAMMPS order and sign, as ahip_compute
 * Steps: upload, ahip_wrap_cell_dev, ahip_borders_cell_dev (retried with a larger capacity when needed), ahip_build_neighbors_dev over the bounding box of the
 * cell's eight corners +- rc, the evaluation of ahip_compute_dev, ghost forces added to their sources, download.  Nothing is reused between calls (ahip_compute_cell_reuse below does that).  A model of more
 * than 16 types takes its active set from the types present.  ahip_last_path, ahip_get_edges and the other accessors keep working afterwards; their rows are the
 * atoms followed by the ghosts, and ahip_last_cell_rows maps every row to its atom (nrows = natoms + ghosts; row_atom: room for nrows entries, or NULL for the
 * count alone). */
int ahip_compute_cell(ahip_model *m, int natoms, const double *x, const int *mtype, const double *cell, const int *pbc, double skin, double *f,
                      double *eatom, double *eng, double *virial);
int ahip_last_cell_rows(ahip_model *m, int *nrows, long long *row_atom);

/* ahip_compute_cell for a caller that hands over nearly the same structure again and again (MD in Python, a relaxation, NEB images, a variable-cell optimiser):
 * the model keeps the ghosts and the neighbor list of one call and the next call runs on them when that is provably safe.  Arguments, output contract, argument
 * errors and the handling of the float16-range alarm are those of ahip_compute_cell; *rebuilt (may be NULL) receives 1 when the call built ghosts and list
 * (exactly the steps of ahip_compute_cell), 0 when it ran on the held ones.  Opt-in: ahip_compute_cell itself keeps nothing.
 * Held after a rebuild: the cell A0, the wrapped atom positions xhold, per ghost its source atom and its integer image n (recovered on the device from the
 * shifts as round(shift . A0^-1)), the installed list, and host copies of mtype, pbc, skin and natoms.
 * A call tries the held list when one exists and is still the installed list, natoms, every mtype[i], pbc and skin equal the held ones, and skin > 0 (with
 * skin = 0 every call rebuilds).  It uploads x and rewrites every row on the device (one kernel, one thread per row): with A the cell of THIS call,
 *     t = (x_a - xhold_a) . A^-1,   k_d = floor(t_d + 0.5) on periodic axes, 0 on open ones      (the caller may have wrapped the atom in between, or not)
 *     atom row a = x_a - k . A,     ghost row (a, n) = x_a - k . A + n . A
 * so every ghost is an exact periodic image in the new cell.  The largest |x_a - k . A - xhold_a| = U comes back in one 4-byte read-back (squared, in float32,
 * rounded up).  Then the evaluation of ahip_compute_dev runs on the refreshed rows with the held list; the edge build filters the list at the model's own
 * cutoffs in every call, as it does for LAMMPS' skin-inflated list.  One synchronisation for U and the final one, where a rebuild has three.
 * CRITERION.  rc = largest model cutoff + skin; h0_d the heights of the HELD cell; M_d = ceil(rc / h0_d) + 1; g_d = |a_d - a0_d| the Euclidean length of the
 * change of lattice vector d; sums and the minimum over the periodic axes only.  The held list is used iff
 *     2 U + sum_d M_d g_d <= skin      and      sum_d g_d <= min_d h0_d
 * (an unchanged cell: the classic U <= skin / 2; no periodic axis: 2 U <= skin), else the call rebuilds inside itself.
 * Why that is enough: take atom i and image n' of atom j at held distance D0.  Its distance has changed by at most 2 U + sum_d |n'_d| g_d.  The held positions
 * are wrapped, so D0 >= (|n'_d| - 1) h0_d for every d.  If |n'_d| <= M_d on every axis, the change is <= skin < D0 - r_max whenever D0 > rc.  Otherwise let
 * k = max_d (|n'_d| - M_d) >= 1: then D0 >= rc + k h0 on that axis, while the change is <= skin + k sum_d g_d <= skin + k min_d h0_d.  Either way a pair that
 * was outside the held list (D0 > rc) is still outside r_max.
 * The hold ends with ahip_cell_reuse_reset; with anything that installs another list or other rows (ahip_neigh_update*, ahip_build_neighbors_dev,
 * ahip_borders_*_dev, ahip_compute_cell, an ahip_compute_cells with atoms); with any successful ahip_set_option; and with an ahip_compute_cell_reuse that fails
 * behind a launch.  A call refused for its arguments (a singular or non-finite cell included: AHIP_ERR_ARG before any launch) leaves it as it was.
 * ahip_last_cell_rows, ahip_get_edges, ahip_last_path and the other accessors keep working after a call on the held list: the rows are the held rows, the edges
 * those of this evaluation.
 * ahip_cell_reuse_stats: successful ahip_compute_cell_reuse calls, and how many of them rebuilt, since the model was loaded or ahip_cell_reuse_reset was called
 * (either pointer may be NULL).
 * Measured on one MI355X (tools/cell_reuse_cost.py, profiles/cell_reuse_cost.txt): a 200-call random walk of 0.02 A per call at skin 1.0 A, float32 model S,
 * host clock per call: 64-atom Si cell 198.7 us against 393.0 us through ahip_compute_cell (5 calls rebuilt), 10 648-atom Si box 733.7 us against 1019.5 us (7 rebuilt).
 * A variant that enqueues the evaluation before U is known and reads both back in one synchronisation is left as a follow-up. */
int ahip_compute_cell_reuse(ahip_model *m, int natoms, const double *x, const int *mtype, const double *cell, const int *pbc, double skin, double *f,
                            double *eatom, double *eng, double *virial, int *rebuilt);
int ahip_cell_reuse_reset(ahip_model *m);
int ahip_cell_reuse_stats(ahip_model *m, long long *calls, long long *rebuilds);

/* A RELAXATION of the atomic positions at fixed cell in one call: FIRE (Bitzek et al. 2006 as ASE implements it, unit masses) with the optimiser's state on the
 * device.  The host enqueues check_every moves -- each with its evaluation -- without a wait and then reads one small state block back, where a loop over
 * ahip_compute_cell_reuse pays an upload, three downloads and two synchronisations per move.  HOST pointers; arguments and argument errors are those of
 * ahip_compute_cell_reuse, and besides: skin <= 0, p == NULL or a parameter outside the range given below.  All of them are AHIP_ERR_ARG before any launch, with x
 * untouched and a held list as it was.
 *   x      [natoms][3]  in: the start; out: the relaxed positions, NEVER wrapped (an atom that leaves the cell keeps its continuous coordinate)
 *   fixed  [natoms] or NULL: non-zero = the atom does not move.  Its force is reported as the model gives it, not zeroed.
 *   f, eatom (or NULL), eng, virial (or NULL): those of the returned x, with the contract of ahip_compute_cell
 *   steps: moves made;  converged: max_i |F_i| <= fmax over the free atoms, from the forces handed out;  fmax_out: that maximum;  evaluations: every
 *   ahip_compute_dev issued, those whose forces were discarded included;  rebuilds: ghost shells and lists built, the first included.  Each may be NULL.
 * Parameters: fmax >= 0; max_steps >= 0; check_every >= 1; 0 < dt_start <= dt_max; max_step > 0; n_min >= 0; f_inc >= 1; 0 < f_dec <= 1; 0 <= alpha_start <= 1;
 *   0 < f_alpha <= 1; all finite.
 * ALGORITHM.  F: the forces with the ghost forces folded home, rows of fixed atoms set to 0.  v = 0, dt = dt_start, alpha = alpha_start, npos = 0 at the start.
 * vf = sum v.F, ff = sum F.F, vv = sum v.v over all atoms.  U: the largest displacement of an atom from where it was when the held list was built (as in
 * ahip_compute_cell_reuse: squared, in float32, rounded up); max_i |F_i|^2 is taken in float32 as well.  Before every move, in this order:
 *   1. U is not finite                          -> NONFINITE
 *   2. 2 U > skin                               -> NEED_REBUILD (the forces just computed are discarded; the cell does not change, so this is the reuse criterion)
 *   3. vf, ff, vv or max |F_i|^2 is not finite  -> NONFINITE
 *   4. max_i |F_i| <= fmax                      -> CONVERGED
 * Otherwise the atoms move:
 *   vf > 0:  c1 = 1 - alpha;  c2 = alpha sqrt(vv / ff);  if npos > n_min: dt = min(dt f_inc, dt_max), alpha *= f_alpha;  then npos += 1
 *   else:    c1 = c2 = 0;  alpha = alpha_start;  dt *= f_dec;  npos = 0
 *   and with the new dt:   v' = c1 v + (c2 + dt) F;   s = min(1, max_step / |dr|);   x' = x + s dt v';   v' is kept unscaled.
 * |dr| is ASE's |dt v'|, the length of the whole 3 natoms vector.  Since v' is linear in v and F,
 *     |dr|^2 = dt^2 (c1^2 vv + 2 c1 (c2 + dt) vf + (c2 + dt)^2 ff),
 * so the three sums decide the move and one reduction pass per move suffices.  (v starts at 0, so the first move takes the else branch: dt_start f_dec.)
 * DEVICE.  k_relax_gather writes [v.F, F.F, v.v] and the float32 bits of |F_i|^2 per atom; the deterministic column sum and the integer maximum of csrc/prims.hip
 * reduce them; k_relax_decide, one thread, applies the above to the state block; k_relax_move, one thread per row (atoms, then ghosts), recomputes x' of the row's
 * source atom and writes the row as the exact periodic image ahip_compute_cell_reuse would write, so the held list serves as it does there.  x and v alternate
 * between two buffers: no thread reads what another thread of the same launch writes.  Once the status is not RUNNING every one of these kernels returns at once:
 * positions, rows and state stay those whose forces the last evaluation of the chunk computes again.
 * HOST.  Rebuild (rows, list, hold as in ahip_compute_cell_reuse), evaluate; then min(check_every, moves left) times {gather, reduce, decide, move, zero f,
 * ahip_compute_dev, ghost forces home} without a wait, and one read-back of the state block.  RUNNING: the next chunk.  NEED_REBUILD: the rows, the list and
 * the hold are built again from the positions on the device, which are evaluated, and the moves go on with v, dt, alpha and npos as they were.  CONVERGED: done.
 * NONFINITE, or the float16-range alarm of any evaluation of the chunk: under fused_arith=auto on the f16x2 arithmetic, once per call, the model degrades to the float32 instance and the
 * positions of the last valid move are evaluated again; otherwise the call returns AHIP_ERR_STATE and nothing is written to x or f (two coincident atoms end
 * so).  An explicit active set that leaves out a type in use is AHIP_ERR_ARG behind the first read-back, nothing written.  A larger check_every wastes up to
 * check_every - 1 evaluations at a rebuild or at convergence and saves a synchronisation per move; the result does not depend on it beyond the rounding of the
 * forces' accumulation order.
 * On success the model holds the list of the last rebuild as ahip_compute_cell_reuse would, with the same skin: a trajectory may go on from the returned x.
 * ahip_last_cell_rows, ahip_get_edges and ahip_last_path describe the last evaluation.  A failure behind a launch ends the hold.
 * Measured on one MI355X (tools/relax_cost.py, profiles/relax_cost.txt): a 200-move run from a 0.05 A jitter at skin 1.0 A, fmax 0, float32 model S, host
 * clock per move, against the same FIRE written in numpy over Calculator(reuse=True).compute: 64-atom Si cell 148.4 / 131.4 / 137.4 us at check_every 1 / 4 / 16
 * against 230.4 us (6 rebuilds; 211 / 220 / 244 evaluations), 10 648-atom Si box 517.9 / 457.2 / 452.3 us against 1632.0 us (2 rebuilds; 203 / 204 / 204
 * evaluations).  Not slower than the Python loop at either size; the end points of the two routes agree to 1e-14 A. */
typedef struct ahip_relax_params {
  double fmax;        /* converged when max_i |F_i| <= fmax (eV/A); >= 0 */
  int    max_steps;   /* moves at most; >= 0 */
  int    check_every; /* moves enqueued between two looks of the host at the state; >= 1 */
  double dt_start, dt_max, max_step;            /* 0.1, 1.0, 0.2 */
  int    n_min;                                 /* 5 */
  double f_inc, f_dec, alpha_start, f_alpha;    /* 1.1, 0.5, 0.1, 0.99 */
} ahip_relax_params;
int ahip_relax_params_default(ahip_relax_params *p);   /* the values above; fmax 0.05, max_steps 500, check_every 4 */
int ahip_relax_cell(ahip_model *m, int natoms, double *x, const int *mtype, const double *cell, const int *pbc, double skin, const int *fixed,
                    const ahip_relax_params *p, double *f, double *eatom, double *eng, double *virial, int *steps, int *converged, double *fmax_out,
                    int *evaluations, int *rebuilds);

/* A RELAXATION of the atomic positions AND THE CELL in one call: the FIRE of ahip_relax_cell over natoms + 3 rows, the strain degrees of freedom among them, with
 * the optimiser's state -- the cell included -- on the device.  HOST pointers; arguments, argument errors and the parameters of `fire` are those of
 * ahip_relax_cell, and besides: an open axis (a slab is relaxed with the strain mask, not with an open axis), cell_out == NULL, smax < 0, cell_factor < 0, or a
 * pressure, smax or cell_factor that is not finite.  All of them are AHIP_ERR_ARG before any launch, with x untouched and a held list as it was.
 *   cell      [9]  in: A0, rows = lattice vectors;   cell_out [9]: the relaxed cell
 *   x         in: the start; out: the relaxed positions in cell_out, NEVER wrapped
 *   f, eatom (or NULL), eng, virial (or NULL): those of the returned x in cell_out, with the contract of ahip_compute_cell
 *   steps, converged, fmax_out, evaluations, rebuilds: as in ahip_relax_cell;  smax_out: max_ab |W_ext,ab| / V of the returned configuration;  converged: both
 *   conditions below, from the forces and the virial handed out.  Each may be NULL.
 * STATE.  A deformation gradient D (3 x 3, D = I at the start) and reference coordinates q_i (q_i = x_i at the start).  The configuration is A = A0 D^T (row
 * a_d = D a0_d) and x_i = D q_i.  The generalised coordinates are the natoms + 3 rows (q_1 .. q_n, c D), c = cell_factor, 0 meaning natoms.
 * GENERALISED FORCES.  W: the symmetric virial matrix of the evaluation in the sign this library reports (W = -dE/d(strain)); V = |det A|;
 *   W_ext = W - pressure V I;   hydrostatic: W_ext = (tr W_ext / 3) I;   then W_ext,ab = 0 wherever mask (xx, yy, zz, xy, xz, yz) is 0.
 *   atoms:  G_i = D^T F_i, 0 for a fixed atom (which follows the cell affinely: its q never changes);   strain rows:  G_D = W_ext D^-T / c
 * These are -dH/dq_i and -dH/d(c D) of H = E + pressure V at fixed q resp. fixed D (mask and hydrostatic project the latter).
 * FIRE is that of ahip_relax_cell with F replaced by G and v by the velocities of the natoms + 3 rows: vf = sum v.G, ff = sum G.G, vv = sum v.v, c1, c2, dt, alpha,
 * npos, |dr| and s = min(1, max_step / |dr|) exactly as stated there.  Then v' = c1 v + (c2 + dt) G for every row, q' = q + s dt v' and D' = D + s dt v'_D / c.
 * U is the displacement ahip_compute_cell_reuse would measure for x = D q in the cell A against the rows of the last rebuild (minimum image in A; squared, in
 * float32, rounded up); g_d = |a_d - a_d(hold)| against the cell of the last rebuild, M_d and h0_d those of that cell.  Before every move, in this order:
 *   1. U is not finite                                                          -> NONFINITE
 *   2. not (2 U + sum_d M_d g_d <= skin and sum_d g_d <= min_d h0_d)            -> NEED_REBUILD (the forces just computed are discarded)
 *   3. vf, ff, vv, max |F_i|^2, V, W_ext or det D is not finite, or det D <= 0  -> NONFINITE
 *   4. max_i |F_i| <= fmax (Cartesian forces, free atoms) and max_ab |W_ext,ab| / V <= smax (eV/A^3)   -> CONVERGED
 *   5. the move; but if det D' is not finite or <= 0, or A0 D'^T is singular, nothing moves            -> NONFINITE
 * When max_steps moves are made, the configuration of the last one passes 1-4 once more without a move, so what is handed out was evaluated on a list that
 * holds for it (a rebuild there evaluates it again).
 * DEVICE.  k_vcell_gather writes G_i, [v.G, G.G, v.v] and the float32 bits of the Cartesian |F_i|^2 per atom; k_vcell_decide, one thread, adds the nine strain
 * terms from the virial the evaluation left on the device, decides, and writes the coefficients, D', v'_D and the geometry (cell, inverse) of A0 D'^T into the
 * state block -- the host has not seen that cell; k_vcell_move, one thread per row (atoms, then ghosts), recomputes q' and v' of the row's source atom, forms
 * x' = D' q' and writes the row as the exact periodic image in A' that ahip_compute_cell_reuse would write.  q and v alternate between two buffers; no thread
 * reads what another thread of the same launch writes; once the status is not RUNNING every kernel returns at once.
 * HOST.  The loop of ahip_relax_cell.  At NEED_REBUILD the host takes the cell from the state block it has just read, forms x = D q on the device and builds rows,
 * list and hold in that cell; the moves go on with v, v_D, dt, alpha and npos as they were.  NONFINITE, the float16-range alarm and an inactive type: as there
 * (AHIP_ERR_STATE resp. AHIP_ERR_ARG, nothing written to x, cell_out or f); a cell_factor far too small for max_step ends so, by decision 5.
 * On success the model holds the list of the last rebuild: ahip_compute_cell_reuse at the returned x and cell_out with the same skin runs on it.
 * A model without an equilibrium volume (random weights) expands or collapses until a rebuild fails or the atoms leave each other's cutoff: choose a pressure.
 * Measured on one MI355X (tools/vcell_relax_cost.py, profiles/vcell_relax_cost.txt): 200 moves from a 0.05 A jitter at skin 1.0 A, fmax = smax = 0, c = natoms,
 * float32 model S at the virial pressure of the start, host clock per move, against the same algorithm in numpy over Calculator(reuse=True).compute: 64-atom Si cell
 * 247.6 / 238.3 / 343.2 us at check_every 1 / 4 / 16 against 313.3 us (the random-weight model has no stable volume: det D reaches 1.97 with 33 rebuilds on both
 * routes; 265 / 315 / 553 evaluations -- at 16 the evaluations wasted at each rebuild cost more than the synchronisations saved, and the call is slower than the
 * Python loop), 10 648-atom Si box 499.9 / 468.9 / 459.5 us against 1683.5 us (2 rebuilds; 203 / 204 / 204 evaluations).  At the default check_every 4 not slower
 * at either size; the end points of the two routes agree to 1e-14 A (64 atoms) and 5e-8 A (10 648 atoms, float32 forces summed in another order). */
typedef struct ahip_vcell_params {
  ahip_relax_params fire;   /* fmax, max_steps, check_every and the FIRE constants, as in ahip_relax_cell */
  double smax;              /* converged when also max_ab |W_ext,ab| / V <= smax (eV/A^3); >= 0 */
  double pressure;          /* external pressure, eV/A^3; finite */
  double cell_factor;       /* c > 0, or 0 for natoms: the weight of the strain rows among the generalised coordinates */
  int    hydrostatic;       /* non-zero: only the volume changes */
  int    mask[6];           /* xx, yy, zz, xy, xz, yz: 0 = that component of W_ext is not followed */
} ahip_vcell_params;
int ahip_vcell_params_default(ahip_vcell_params *p);   /* ahip_relax_params_default; smax 1e-3, pressure 0, cell_factor 0, not hydrostatic, mask all 1 */
int ahip_relax_vcell(ahip_model *m, int natoms, double *x, const int *mtype, const double *cell, const int *pbc, double skin, const int *fixed,
                     const ahip_vcell_params *p, double *cell_out, double *f, double *eatom, double *eng, double *virial, int *steps, int *converged,
                     double *fmax_out, double *smax_out, int *evaluations, int *rebuilds);

/* MOLECULAR DYNAMICS in one call: NVE (velocity Verlet) or Langevin dynamics (BAOAB, Leimkuhler and Matthews 2013) with the integrator's state on the device.  The
 * host enqueues check_every steps -- each with its evaluation -- without a wait and then reads one small state block back, where a loop over
 * ahip_compute_cell_reuse pays an upload, three downloads and two synchronisations per step.  HOST pointers; arguments and argument errors are those of
 * ahip_relax_cell, and besides: a parameter outside the range given below, v or mass NULL, a mass that is not finite and positive, a v that is not finite,
 * frames != NULL with frame_every == 0 or the reverse, and frames that would take more than 1 GiB on the device (call again with fewer steps and carry x, v and
 * step0 over).  All of them are AHIP_ERR_ARG before any launch, with x, v and f untouched and a held list as it was.
 *   x, v   [natoms][3]  in: the start; out: the state after nsteps steps.  x is NEVER wrapped, as in ahip_relax_cell.
 *   mass   [natoms], per atom
 *   fixed  [natoms] or NULL: non-zero = the atom keeps x, has v = 0 and is left out of ke.  Its force is reported as the model gives it.
 *   f, eatom (or NULL), eng, virial (or NULL): those of the returned x, with the contract of ahip_compute_cell
 *   thermo [nsteps / sample_every + 1][8] or NULL: {pe, ke, vxx, vyy, vzz, vxy, vxz, vyz} of the configurations 0, sample_every, 2 sample_every, ...
 *   frames [nsteps / frame_every + 1][natoms][3], unwrapped positions of the configurations 0, frame_every, ...; NULL iff frame_every == 0
 *   evaluations, rebuilds (each may be NULL): as in ahip_relax_cell
 * natoms == 0 launches nothing: eng, virial and the thermo rows are 0.
 * ALGORITHM.  BAOAB.  hdtf = 0.5 dt ftm2v, c1 = exp(-gamma dt) and c2 = sqrt(1 - c1^2) are formed on the host in double; gamma = 0 gives c1 = 1, c2 = 0: velocity
 * Verlet with two half drifts.  The device holds the unwrapped x and the post-thermostat velocity w in two buffers each, as the relaxation does (w = v at the
 * start), vnow [natoms][3], mass, the mask, an MdState block, the thermo rows and the frames.  With the forces F_n of configuration n on the device
 * (n = 0 .. nsteps), each iteration runs three kernels.
 * 1. k_md_gather, one thread per atom: v_n = w + (n > 0 ? hdtf F_n / m : 0), 0 for a fixed atom.  It writes vnow, m |v_n|^2 and the float32 bits of |F_i|^2 as
 *    k_relax_gather does, and the frame row when n % frame_every == 0.  prim_sum_columns_f64 and prim_max_i32 then reduce these, and the displacement bits the
 *    move before left.
 * 2. k_md_decide, one thread, the only device writer of the state.  In this order:
 *      1. U is not finite                              -> NONFINITE
 *      2. 2 U > skin                                   -> NEED_REBUILD (the forces just computed are discarded and no thermo row is written)
 *      3. the ke sum, max |F_i|^2 or pe is not finite  -> NONFINITE
 *      4. n % sample_every == 0: thermo row n / sample_every is written; pe and the virial are the 7 doubles the evaluation left on the device,
 *         ke = 0.5 mvv2e sum_i m_i |v_n,i|^2
 *      5. n == nsteps                                  -> DONE
 *      6. otherwise n += 1 and the move happens.
 * 3. k_md_move, one thread per row (atoms, then ghosts), on the row's source atom a, out of configuration n (the n of before decision 6):
 *      v' = vnow_a + hdtf F_a / m_a;   xh = x_a + 0.5 dt v';   w' = gamma > 0 ? c1 v' + c2 sqrt(kT / (m_a mvv2e)) xi(a, step0 + n) : v';   x' = xh + 0.5 dt w'
 *    (a fixed atom: x' = x_a, w' = 0).  The row is written as the exact periodic image, the way k_relax_move writes it; atom rows also store x', w' and the
 *    displacement bits.  No thread reads what another thread of the same launch writes.
 * Once the status is not RUNNING, all three kernels return at once.
 * NOISE.  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85), key (seed lo32, seed hi32), counter (atom lo32, step lo32,
 * step hi32, j), j = 0, 1.  From the output words (w0, w1, w2, w3): u1 = (((uint64)w0 << 21 | w1 >> 11) + 0.5) 2^-53, u2 likewise from w2, w3;
 * z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = sqrt(-2 ln u1) sin(2 pi u2);  xi = (z0, z1 of j = 0; z0 of j = 1).  The noise of a step depends only on (seed, atom,
 * step): not on check_every, on rebuilds, on the degradation replay, on ghost threads recomputing it, or on how a trajectory is cut into calls.  With gamma = 0
 * no random number is drawn.  ahip_debug_md_noise runs exactly this device function for atoms 0 .. n-1 (out [n][3], HOST).
 * HOST.  The loop of ahip_relax_cell: rebuild rows, list and hold from x, evaluate; per chunk min(check_every, steps left) times {gather, reduce, decide, move,
 * zero f, evaluation, ghost forces home} without a wait, then one read-back of the state block.  The step count is known in advance, so iteration n == nsteps is
 * enqueued as gather, reduce, decide only, behind the last move's evaluation, with no evaluation behind it: what is handed out was evaluated on a list that
 * holds for it.  NEED_REBUILD: rows, list and hold are built from the positions on the device, which are evaluated; w and n stay as they were.  NONFINITE, the
 * float16-range alarm and an inactive type: exactly as in ahip_relax_cell (one degradation to the float32 instance under fused_arith=auto; otherwise
 * AHIP_ERR_STATE resp. AHIP_ERR_ARG with nothing written to x, v or f).  At the end v is vnow.  At check_every = 1 the evaluations are
 * nsteps + 1 + 2 (rebuilds - 1), minus one when the final check was what rebuilt.
 * On success the model holds the list of the last rebuild: ahip_compute_cell_reuse at the returned x with the same skin runs on it, and a following ahip_md_cell
 * with the returned x, v and step0 + nsteps continues the trajectory (its first thermo row is this call's last).  A failure behind a launch ends the hold.
 * Measured on one MI355X (tools/md_cost.py, profiles/md_cost.txt): 200 steps of 0.001 ps from 300 K and a 0.05 A jitter at skin 1.0 A, float32 model S, a thermo
 * row per step, host clock per step, against the same BAOAB written in numpy over Calculator(reuse=True).compute.  64-atom Si cell: NVE 178.8 / 151.5 / 150.8 us at
 * check_every 1 / 4 / 16 against 259.9 us (7 rebuilds; 213 / 227 / 247 evaluations), Langevin (gamma 5 / ps) 159.3 / 138.0 / 141.1 us against 246.5 us (6 rebuilds;
 * 211 / 218 / 238 evaluations).  10 648-atom Si box: NVE 551.7 / 533.5 / 619.9 us against 1555.0 us (9 rebuilds; 217 / 228 / 273 evaluations), Langevin 527.9 / 519.9 /
 * 578.3 us against 1903.1 us (8 rebuilds; 215 / 223 / 253 evaluations).  At the default check_every 4 not slower than the Python loop at either size; at 16 the
 * evaluations wasted at each rebuild cost more than the synchronisations saved.  The NVE end points of the two routes agree to 2e-14 A. */
typedef struct ahip_md_params {
  int    nsteps;        /* steps to make; >= 0 */
  int    check_every;   /* steps enqueued between two looks of the host at the state; >= 1 */
  int    sample_every;  /* a thermo row at steps 0, sample_every, 2 sample_every, ... <= nsteps; >= 1 */
  int    frame_every;   /* a frame of positions at those steps; 0 = none */
  double dt;            /* > 0 */
  double ftm2v, mvv2e;  /* unit factors as in LAMMPS: a = ftm2v F / m, ke = 0.5 mvv2e m v^2; both > 0 */
  double gamma;         /* friction, 1 / time; 0 = NVE (no random number is drawn) */
  double kT;            /* bath temperature in energy units; >= 0; read only when gamma > 0 */
  unsigned long long seed, step0;   /* noise key; index of this call's first step (continuing a trajectory) */
} ahip_md_params;
int ahip_md_params_default(ahip_md_params *p);   /* metal units, dt 0.001 ps, gamma 0, check_every 4, sample_every 1, frame_every 0 */
int ahip_md_cell(ahip_model *m, int natoms, double *x, double *v, const int *mtype, const double *mass, const double *cell, const int *pbc,
                 double skin, const int *fixed, const ahip_md_params *p, double *f, double *eatom, double *eng, double *virial,
                 double *thermo, double *frames, int *evaluations, int *rebuilds);
int ahip_debug_md_noise(unsigned long long seed, unsigned long long step, int n, double *out /* [n][3] */);

/* MOLECULAR DYNAMICS AT CONSTANT PRESSURE in one call: the BAOAB of ahip_md_cell inside an isotropic stochastic cell rescaling (Bernetti and Bussi, J. Chem. Phys.
 * 153, 114107 (2020), in its epsilon = ln V form, Euler step), with the integrator's state, the barostat's decision, the cell and its inverse on the device: the
 * host does not look between steps.  HOST pointers; arguments, argument errors, md.* and the outputs are those of ahip_md_cell, and besides: an open axis,
 * natoms == 0, cell_out == NULL, a pressure that is not finite, a compressibility or tau_p that is not finite and > 0, frame_cells != NULL with frame_every == 0
 * (it may be NULL otherwise), and md.kT, which is ALWAYS read because it sets the barostat's noise: kT = 0 gives the deterministic (Berendsen-limit) barostat,
 * gamma = 0 keeps the particles on velocity Verlet.  All of them are AHIP_ERR_ARG before any launch, with x, v, cell_out and f untouched and a held list as it was.
 *   cell      [9]  in: the start, rows = lattice vectors;   cell_out [9]: the cell after nsteps steps
 *   x, v      in: the start; out: the state after nsteps steps in cell_out.  x is NEVER wrapped.
 *   fixed     non-zero = the atom follows the cell affinely (its reduced coordinates never change, as a fixed atom of ahip_relax_vcell), has v = 0, no part in ke
 *   f, eatom (or NULL), eng, virial (or NULL): those of the returned x in cell_out
 *   thermo [nsteps / sample_every + 1][10] or NULL: {pe, ke, vxx, vyy, vzz, vxy, vxz, vyz, V, P};   frames as in ahip_md_cell;
 *   frame_cells [nsteps / frame_every + 1][9] or NULL: the cell of every frame
 * ALGORITHM.  Configuration n has the cell A_n, the forces F_n and the virial W_n (in the sign this library reports, as W_ext = W - p V I of ahip_relax_vcell
 * uses it) of its evaluation.  U, g_d, M_d and h0_d are those of ahip_relax_vcell: the displacement by minimum image in A_n against the rows of the last rebuild
 * (squared, float32, rounded up), g_d = |a_d - a_d(hold)| against the cell of the last rebuild.  Each iteration runs three kernels.
 * 1. k_npt_gather, one thread per atom: v_n and what goes with it, exactly as k_md_gather.  The reductions follow.
 * 2. k_npt_decide, one thread, the only device writer of the state.  In this order:
 *      1. U is not finite                                                          -> NONFINITE
 *      2. not (2 U + sum_d M_d g_d <= skin and sum_d g_d <= min_d h0_d)            -> NEED_REBUILD (the forces just computed are discarded, no thermo row is
 *         written and nothing advances)
 *      3. the ke sum, max |F_i|^2, pe, V = |det A_n| or P is not finite, or V <= 0 -> NONFINITE;   ke = 0.5 mvv2e sum_i m_i |v_n,i|^2,
 *         P = (2 ke + W_xx + W_yy + W_zz) / (3 V)
 *      4. n % sample_every == 0: the thermo row;  n % frame_every == 0: the frame's cell
 *      5. n == nsteps                                                              -> DONE
 *      6. d eps = -(beta_T / tau_p) (P0 - P) dt + sqrt(2 kT beta_T dt / (V tau_p)) xi_V(step0 + n);   mu = exp(d eps / 3);   A_n+1 = mu A_n entry by entry.
 *         If mu is not finite or A_n+1 is singular, nothing moves                  -> NONFINITE
 *         else mu, A_n+1 and its inverse go into the state block, n += 1 and the move happens.
 * 3. k_npt_move, one thread per row (atoms, then ghosts), on the row's source atom a: (x', w') of k_md_move, then x'' = mu x', w'' = w' / mu (a fixed atom:
 *    x'' = mu x_a, w'' = 0).  The row is written as the exact periodic image in A_n+1 against the rows of the last rebuild, the way k_vcell_move writes it, with
 *    the displacement bits rounded up.  No thread reads what another thread of the same launch writes.
 * Once the status is not RUNNING, all three kernels return at once.
 * NOISE.  xi_V(step) is the first component of the xi of ahip_md_cell at the atom word 0xFFFFFFFF (natoms is an int: no atom has it).  It depends on (seed, step)
 * only: not on check_every, on rebuilds, on the degradation replay, or on how a trajectory is cut into calls.  With kT = 0 it is not drawn.
 * ahip_debug_npt_noise runs exactly this device function (out [1], HOST).
 * HOST.  The loop of ahip_md_cell.  At NEED_REBUILD the host takes the cell from the state block it has just read and builds rows, list and hold from the device
 * positions in that cell; w and n stay as they were.  NONFINITE, the float16-range alarm and an inactive type: exactly as in ahip_md_cell (nothing written to x, v,
 * cell_out or f).  The final iteration is gather, reduce, decide only.  The evaluation count follows the rule stated there.
 * On success the model holds the list of the last rebuild: ahip_compute_cell_reuse at the returned x and cell_out with the same skin runs on it, and a following
 * ahip_npt_cell with the returned x, v, cell_out and step0 + nsteps continues the trajectory (its first thermo row is this call's last).
 * DEFAULTS.  compressibility 1.6 A^3/eV (a bulk modulus of 100 GPa = 0.624 eV/A^3: a typical metal or semiconductor; water is some 70 A^3/eV); tau_p 1 ps.  Only
 * beta_T / tau_p enters the drift, so a wrong compressibility merely rescales the relaxation time.
 * Measured on one MI355X (tools/npt_cost.py, profiles/npt_cost.txt): 200 steps of 0.001 ps from 300 K and a 0.05 A jitter at skin 1.0 A, float32 model S at
 * the virial pressure of the start, beta_T 1.6 A^3/eV, tau_p 0.1 ps, a thermo row per step, host clock per step, against the same algorithm in numpy over
 * Calculator(reuse=True).compute (the random-weight model has no stable volume: V / V0 reaches 1.12 to 1.13 on both routes).  64-atom Si cell: deterministic
 * barostat over velocity Verlet 174.6 / 155.3 / 188.1 us at check_every 1 / 4 / 16 against 263.7 us (10 rebuilds; 219 / 233 / 313 evaluations), stochastic barostat
 * over Langevin (gamma 5 / ps) 170.8 / 152.6 / 177.6 us against 260.4 us (9 rebuilds; 217 / 229 / 293 evaluations).  10 648-atom Si box: deterministic 633.9 /
 * 657.6 / 1005.7 us against 1511.1 us (26 rebuilds; 251 / 276 / 450 evaluations), stochastic 648.3 / 668.0 / 1019.7 us against 1944.2 us (25 rebuilds; 248 / 272 /
 * 446 evaluations).  At the default check_every 4 not slower than the Python loop at either size (1.70x, 1.71x, 2.30x, 2.91x); a cell that grows this fast rebuilds
 * every 8 steps, so on the large box check_every 1 is the fastest and 16 wastes more evaluations than it saves synchronisations, while staying faster than the
 * loop.  The deterministic end points (positions and cell) of the two routes agree to 9e-15 A (64 atoms) and 5e-9 A (10 648 atoms, float32 forces summed in
 * another order). */
typedef struct ahip_npt_params {
  ahip_md_params md;        /* everything of ahip_md_cell, same meaning and ranges; kT is always read */
  double pressure;          /* P0, energy / volume (metal: eV/A^3); finite */
  double compressibility;   /* beta_T, volume / energy; > 0, finite */
  double tau_p;             /* barostat relaxation time; > 0, finite */
} ahip_npt_params;
int ahip_npt_params_default(ahip_npt_params *p);   /* ahip_md_params_default; pressure 0, compressibility 1.6 A^3/eV, tau_p 1 ps */
int ahip_npt_cell(ahip_model *m, int natoms, double *x, double *v, const int *mtype, const double *mass, const double *cell, const int *pbc,
                  double skin, const int *fixed, const ahip_npt_params *p, double *cell_out, double *f, double *eatom, double *eng, double *virial,
                  double *thermo /* [.][10] */, double *frames, double *frame_cells /* [.][9] */, int *evaluations, int *rebuilds);
int ahip_debug_npt_noise(unsigned long long seed, unsigned long long step, double *out /* [1] */);

/* A BATCH of structures in one call: what ahip_compute_cell computes for each of `nstruct` structures alone, with one upload, one ghost build, one neighbor
 * list and one evaluation for all of them (a data set of small cells is launch- and synchronisation-bound one structure at a time).  HOST pointers.
 *   first  [nstruct + 1], first[0] = 0, non-decreasing: structure s owns the atoms first[s] .. first[s+1] - 1 (an empty structure is allowed; nstruct == 0 too)
 *   x      [first[nstruct]][3], mtype [first[nstruct]]      cells [nstruct][9], pbc [nstruct][3]: per structure, the conventions of ahip_compute_cell
 *   f, eatom (or NULL): WRITTEN in the caller's atom order, ghost forces already added to their sources
 *   eng    [nstruct];  virial [nstruct][6] or NULL: xx,yy,zz,xy,xz,yz in LAMMPS order and sign.  An empty structure gives 0.
 * How: every structure keeps its own frame for the wrap and for its ghost images (per structure exactly the rows, order, sources and shifts of
 * ahip_borders_cell_dev; one scan over all atoms).  Before the list build every row is translated by its structure's origin: uniform slots of the largest extent
 * of any structure plus rc + 1e-6 on a near-cubic grid, so that the batch is ONE non-periodic cloud in which no edge joins two structures (the model is
 * translation-invariant, positions and edge vectors are float64).  eng[s] is the sum of the per-atom energies of s; virial[s] is the sum of x_row (x) F_row over
 * the atoms and ghosts of s in its own frame, before the ghost forces go home -- the same number on every kernel path.  Three synchronisations besides the staged
 * copies (one packed upload; the downloads of the sums, f, eatom and the ghost sources, each of which waits for its own copy): the ghost total, the one inside
 * the list build, the final one.
 * Errors are AHIP_ERR_ARG before any launch and before anything is written, and name the structure: a singular or non-finite cell, a non-finite position, a type
 * outside the model's, `first` not non-decreasing, atoms + images beyond 2^31 - 1 rows.  One error comes late, behind the evaluation, with eng / virial already
 * zeroed and f not written: an explicit active set (ahip_set_active_types) that leaves out a type in use (AHIP_ERR_ARG), like the float16-range alarm below.  RULE: the list is binned over all slots, so a very uneven batch (one
 * large cell among many small ones) wastes bins; when the grid would exceed 2^26 bins the call returns AHIP_ERR_ARG with "split the batch" in the message --
 * call again with fewer, or more even, structures.  The float16-range alarm is handled as in ahip_compute_cell: under fused_arith=auto the WHOLE batch is
 * evaluated again on the float32 instance; under an explicit f16x2 the call returns AHIP_ERR_STATE and f is not written.  A model of more than 16 types takes its
 * active set from the union of the types present.  ahip_last_path, ahip_get_edges and ahip_last_cell_rows keep working: the rows are all atoms of the batch
 * followed by all ghosts (grouped by structure, in order), row_atom is the atom's index in the batch.  ahip_last_cells_ghosts gives the ghosts per structure of
 * the last batch (nghost: room for nstruct entries, or NULL for the count alone).  Both are set when a call has SUCCEEDED: a call refused for its arguments leaves
 * them as they were, a call that fails later leaves nothing to report (AHIP_ERR_STATE from both until the next success).  ahip_last_cells_ghosts is not reset by
 * a later ahip_compute_cell: it keeps describing the last successful batch.  A batch without atoms launches nothing: rows and ghost counts are 0, while the
 * neighbor list and the edges (ahip_get_edges) stay those of the evaluation before. */
int ahip_compute_cells(ahip_model *m, int nstruct, const int *first, const double *x, const int *mtype, const double *cells, const int *pbc, double skin,
                       double *f, double *eatom, double *eng, double *virial);
int ahip_last_cells_ghosts(ahip_model *m, int *nstruct, long long *nghost);

/* v += dtf*f/m ; x += dt*v  style velocity-Verlet half steps on device arrays (NVE).
 *   mode 0: v += 0.5*dt*f*ftm2v/mass[type]; x += dt*v      (initial_integrate)
 *   mode 1: v += 0.5*dt*f*ftm2v/mass[type]                  (final_integrate)
 * mass_by_mtype: HOST [num_types], indexed by (full) model type; any number of types (up to 16 travel in the kernel arguments, more in a small device
 * table that is uploaded when its content changes, which synchronises `stream` once). */
int ahip_nve_dev(ahip_model *m, int mode, int n, double *x_dev, double *v_dev, const double *f_dev,
                 const int *mtype_dev, const double *mass_by_mtype, double dt, double ftm2v, void *stream);
/* mode 0 for the nlocal owned atoms AND f[0 .. nall) = 0 behind it (the array the next force evaluation accumulates into, pair_nequip_allegro.cpp:370-377
 * adds to whatever f holds): one launch instead of an integrate and a zero-fill per step of the stand-alone driver. */
int ahip_nve_first_dev(ahip_model *m, int nlocal, int nall, double *x_dev, double *v_dev, double *f_dev, const int *mtype_dev,
                       const double *mass_by_mtype, double dt, double ftm2v, void *stream);

/* ---- ghost exchange of a spatially decomposed system (csrc/comm.hip) ---------------------------
 * Replaces what the reference gets from LAMMPS: ghost positions through Comm::forward_comm before compute(), and the forces the
 * model puts on ghost atoms (pair_nequip_allegro.cpp:370-377 adds to all nlocal + nghost rows) returned to their owners by the
 * reverse communication of `newton_pair on` (pair_nequip_allegro.cpp:149 requests it, :366-368 relies on it).
 * HIP pack / unpack kernels + RCCL ncclSend / ncclRecv groups on the caller's stream (one group per dimension, both directions);
 * librccl.so is opened at the first RCCL call.  The hosted transport moves the same packed buffers through a host callback
 * (CPU tests through the emulation build; several ranks sharing one GPU). */
typedef struct ahip_comm ahip_comm;
typedef struct ahip_xfer_op {
  int kind;          /* 0 = send, 1 = receive, 2 = in-place all-reduce float64 sum, 3 = in-place all-reduce int32 max */
  int peer;          /* rank (send / receive) */
  void *ptr;         /* the buffer as the library sees it (a device pointer on the GPU) */
  long long bytes;
} ahip_xfer_op;
/* performs all ops of one group (they may only complete together: post the receives before waiting for the sends); 0 = success */
typedef int (*ahip_xfer_fn)(void *user, int nops, const ahip_xfer_op *ops);

/* ncclGetVersion() of the librccl.so the RCCL transport opens (0: not available).  Reporting only (bench.py prints it per rank). */
int ahip_comm_rccl_version(void);

/* 128-byte RCCL unique id (ncclGetUniqueId): rank 0 creates it, the host program hands it to every rank */
int ahip_comm_unique_id(unsigned char id[128]);
int ahip_comm_create_rccl(int rank, int nranks, const unsigned char id[128], int device, ahip_comm **out);
int ahip_comm_create_hosted(int rank, int nranks, ahip_xfer_fn fn, void *user, ahip_comm **out);
void ahip_comm_free(ahip_comm *c);

/* Exchange plan, set after every re-neighboring (LAMMPS Comm::borders): nswaps directed swaps, two per dimension in the order
 * (dim 0: -,+), (dim 1: -,+), (dim 2: -,+).  Swap s sends rows send_idx_dev[s][0..nsend[s]) of x, shifted by shift[s] along dim[s],
 * to sendrank[s] and receives nrecv[s] rows from recvrank[s] into rows [first_recv[s], first_recv[s] + nrecv[s]) of x.  Later swaps
 * may send rows received by earlier dimensions.  The index arrays stay owned by the caller and must live until the next plan. */
int ahip_comm_set_plan(ahip_comm *c, int nswaps, const int *dim, const int *sendrank, const int *recvrank, const double *shift,
                       const int *nsend, const int *nrecv, const int *first_recv, const long long *const *send_idx_dev);
/* One rank: ghost g (row nlocal + g) is the image of local row src_dev[g] displaced by shift_dev[g][3]. */
int ahip_comm_set_plan_local(ahip_comm *c, int nlocal, int nghost, const long long *src_dev, const double *shift_dev);
/* Re-neighboring inside the library (round 6) -- what LAMMPS' Comm::exchange and Comm::borders give the reference at every re-neighboring
 * (pair_nequip_allegro.cpp:366-368 relies on the ghost shell and the reverse communication they set up).  Brick decomposition: `grid` ranks per dimension,
 * this rank at `coord`, rank = (cx * gy + cy) * gz + cz, brick [lo, hi), periodic `box`.  Both calls are collective over the communicator, synchronise `stream`
 * a few times (counts travel to the host) and agree on overflow TOGETHER (no rank is left waiting in an exchange).
 * ahip_comm_migrate: wraps the nlocal owned positions into the box and hands the atoms that left the brick (at most one brick per re-neighboring) to the
 *   neighbour brick with their velocity, tag and model type; the arrays have room for `capacity` rows; *nlocal_new is the new owned count, or -(rows needed)
 *   on every rank when some brick would overflow (the arrays are then partly migrated: treat as fatal, start with more room).
 * ahip_comm_borders: rebuilds the ghost shell of thickness rc behind the owned rows of x_dev / mtype_dev (capacity rows) by the six directed swaps of
 *   ahip_comm_set_plan -- send lists in ascending row order, later dimensions forwarding what earlier ones received -- and INSTALLS that plan in the communicator
 *   (the lists live in the library until the next call).  *nall = owned + ghost rows; a value above `capacity` means nothing may be used and every rank got that
 *   answer: call again with larger arrays (the owned rows are untouched). */
int ahip_comm_migrate(ahip_comm *c, int nlocal, double *x_dev, double *v_dev, long long *tag_dev, int *mtype_dev, int capacity, const double *box,
                      const int *grid, const int *coord, int *nlocal_new, void *stream);
int ahip_comm_borders(ahip_comm *c, int nlocal, double *x_dev, int *mtype_dev, int capacity, const double *lo, const double *hi, const double *box,
                      double rc, const int *grid, const int *coord, int *nall, void *stream);
/* The same two calls for ANY cell -- triclinic, with open axes -- decomposed into bricks of FRACTIONAL coordinates (LAMMPS' "lamda" decomposition of a triclinic
 * box).  `cell`: host [9], rows = lattice vectors; `pbc`: host [3]; s = x . cell^-1 and m_d = rc / h_d (h_d the cell height along d) are those of
 * ahip_borders_cell_dev (csrc/cell_geom.h), so one rank and many ranks decide alike.  Both calls are collective.
 * Brick: the brick of `coord` is lo_d = (double)coord_d / grid_d <= s_d < hi_d = (double)(coord_d + 1) / grid_d; an atom's brick index along d is
 *   clamp(floor(s_d * grid_d), 0, grid_d - 1), so an atom outside [0, 1) on an open axis belongs to the edge brick.
 * ahip_comm_migrate_cell: wraps the owned rows with the rule of ahip_wrap_cell_dev (periodic axes only; an atom already inside comes back bit for bit), then, per
 *   decomposed dimension, builds the keep / down / up lists with the delta rule of ahip_comm_migrate on the brick index above (at most one brick per
 *   re-neighboring; with two bricks on a periodic axis "down" wins).  Across the face of an open axis nothing leaves and nothing arrives: there the difference of
 *   brick indices is taken without the modulus, and no message is posted between the two edge bricks.  Row order (kept rows, then what the upper neighbour sent
 *   down, then what the lower neighbour sent up), the 64-byte record, the single merged message with two bricks and the overflow answer -(rows needed), agreed on
 *   by all ranks, are those of ahip_comm_migrate.
 * ahip_comm_borders_cell: per dimension, over the rows known before that dimension, the lower list is s_d < lo_d + m_d and the upper list s_d >= hi_d - m_d, with
 *   s taken from the row's current Cartesian position; ghosts are stored as Cartesian rows.  A step that wraps adds the lattice vector +a_d (downwards) or -a_d
 *   (upwards) as three plain additions, a step that does not wrap copies the row bit for bit.  Nothing crosses the face of an open axis: the edge brick's swap towards
 *   the face sends nothing, the brick at the other edge receives nothing through it, and no message is posted between them (with one brick along the axis that
 *   swap has nsend = nrecv = 0).  Append order (first what came from above, then what came from below), the 28 bytes per row, the single merged message with two
 *   bricks and the capacity protocol with its agreement are those of ahip_comm_borders.  The call INSTALLS the plan that ahip_comm_forward / ahip_comm_reverse run;
 *   forward adds the same lattice vectors (a plan of ahip_comm_set_plan or ahip_comm_borders keeps its single-coordinate shift, bit for bit as before).
 * An orthogonal cell (zero off-diagonal entries, positive diagonal) with all three axes periodic IS the box of ahip_comm_migrate / ahip_comm_borders and is decided
 *   by them, in Cartesian coordinates (brick [box_d coord_d / grid_d, box_d (coord_d + 1) / grid_d), single-coordinate shifts), so that both spellings of one system
 *   give the same rows bit for bit; fractional arithmetic cannot promise that (5 * (1 / 24) and 5 / 24 are different doubles).
 * Refusals: AHIP_ERR_ARG before any launch or message, from the host arguments alone, hence on every rank alike (nobody is left waiting):
 *   a singular or non-finite cell, a grid that does not match the communicator (both calls); and, in ahip_comm_borders_cell, where rc is known:
 *   grid_d >= 2 with h_d / grid_d < rc (a brick thinner than the halo), and grid_d == 1 on a periodic axis with h_d < rc (several images per direction: one rank
 *   builds that shell with ahip_borders_cell_dev).  Bricks thinner than the halo, which need several swaps per direction, are out of scope. */
int ahip_comm_migrate_cell(ahip_comm *c, int nlocal, double *x_dev, double *v_dev, long long *tag_dev, int *mtype_dev, int capacity,
                           const double *cell, const int *pbc, const int *grid, const int *coord, int *nlocal_new, void *stream);
int ahip_comm_borders_cell(ahip_comm *c, int nlocal, double *x_dev, int *mtype_dev, int capacity, const double *cell, const int *pbc,
                           double rc, const int *grid, const int *coord, int *nall, void *stream);
/* x_dev [nall][3]: ghost rows refreshed from their owners (forward);  f_dev [nall][3]: ghost rows added to their owners (reverse). */
int ahip_comm_forward(ahip_comm *c, double *x_dev, void *stream);
int ahip_comm_reverse(ahip_comm *c, double *f_dev, void *stream);
/* in-place all-reduce over the ranks: kind 0 = float64 sum, 1 = int32 max (thermo sums, the re-neighboring flag) */
int ahip_comm_allreduce(ahip_comm *c, void *buf_dev, int count, int kind, void *stream);
/* ring send / receive + both all-reduces with known values through every transport entry point; AHIP_ERR_STATE on a wrong value */
int ahip_comm_selftest(ahip_comm *c, int n, void *stream);
/* hipMemsetAsync(ptr, 0, bytes) on the stream (the driver zeroes its force array with it) */
int ahip_fill_zero_dev(void *ptr_dev, long long bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif

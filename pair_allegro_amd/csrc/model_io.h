// Host-side model description + AHIP blob reader (no HIP, no torch).
#pragma once
#include <map>
#include <string>
#include <vector>

namespace ahip {

struct HostTensor {
  std::vector<int> shape;
  std::vector<double> data;
  long long numel() const { long long n = 1; for (int s : shape) n *= s; return n; }
};

struct HostModel {
  std::string model_dtype = "float32";      // "float32" | "float64": the loader refuses anything else
  bool is_f64() const { return model_dtype != "float32"; }
  std::vector<std::string> type_names;
  std::string type_names_joined;            // whitespace separated (reference metadata form)
  double r_max = 0;
  std::vector<double> per_edge_type_cutoff; // [T*T] model index, empty = r_max everywhere
  int num_types = 0, num_bessels = 0, poly_p = 0, l_max = 0, num_layers = 0;
  int S = 0, U = 0, mlp_depth = 0, mlp_width = 0, readout_depth = 0, readout_width = 0;
  double avg_num_neighbors = 1;
  int allow_tf32 = 0;                       // the reference's fifth metadata key (pair_nequip_allegro.cpp:267-270): the model file permits TF32-class matrix arithmetic
  long long seed = 0;
  std::map<std::string, HostTensor> tensors;

  const HostTensor &get(const std::string &name) const;   // throws std::runtime_error
};

// Reads `path` (.nequip.pth zip archive with an allegro_hip.bin member, or bare .ahip blob).
// Throws std::runtime_error with a user-facing message.
HostModel load_model_file(const std::string &path);

// The same model with its widths zero-padded to the fixed widths of a fused kernel (round 6): S scalar features -> SF, U tensor features -> UF (the columns of the
// (l, u) weight vectors move from l U + u to l UF + u), MLP width W -> WF, read-out width R -> RF.  Padded features are exact zeros all the way (no biases, silu(0) = 0,
// zero path weights, zero rows / columns in every linear), so the padded model computes the same energies and forces; needs S <= SF, U <= UF, W <= WF, R <= RF.
HostModel pad_host_model(const HostModel &h, int SF, int UF, int WF, int RF);

// The same model written as an l_max = LF model (LF >= l_max): zero columns for the new l in the embedding / environment weight vectors (column l U + u does not move),
// the `tp` rows moved to the rows of the same (l1, l2, l3) in the larger path list (every new path zero), zero channel-mixing blocks for the new l.  The new tensor
// components are exact zeros through embedding, environment sum, tensor product and mixing, so the lifted model computes the same energies and forces bit for bit in
// float64; it is what lets an l_max = 1 model with more than 32 tensor features run on the 64-feature l_max = 2 kernel (fused_shapes.h).
HostModel lift_host_model(const HostModel &h, int LF);

// The same model restricted to the model types `active` (strictly ascending, each in [0, T)), which take the compact slots 0 .. A - 1: rows active[k] and
// T + active[k] of `tb.w0` (the centre and neighbour one-hot rows) followed by its Bessel rows, `scale`, `shift` and the type names at `active`, the per-pair cutoffs
// at active x active (an empty matrix stays empty), num_types = A; every other tensor untouched.  A type enters the model nowhere else, so the atoms of a system
// that uses only these types see exactly this model (float64: bit for bit).  Throws std::runtime_error when `active` is not strictly ascending or out of range.
HostModel subset_host_model(const HostModel &h, const std::vector<int> &active);

// Parses an in-memory blob.
HostModel parse_blob(const unsigned char *p, size_t n, const std::string &origin);

}  // namespace ahip

"""Path-difference parity: shared by the CPU harness (tests/test_path_parity.py, emulated layer-at-a-time kernels) and the GPU tests
(tests/test_gpu_path_parity.py, every fused kernel and the layer-at-a-time float32 kernels).

The summed-force bars of the parity tests (5e-4, max|dF| < 1e-4) are blind to one wrong tensor-product coefficient: a 1 % error in one
Clebsch-Gordan entry moves the forces of model L by ~1e-6.  Isolating one path makes it visible: for a model M, a layer k and a path p of
l{k}.tp, the variant M+ carries row p times a boost b, the variant M0 carries row p = 0, and

    Delta = F(M+) - F(M0)        (likewise the per-atom energies and the virial)

is what path p contributes.  The kernel's Delta must match the float64 oracle's to BAR * max|Delta_oracle|; the same error in one entry is
then a ~1e-3 relative change of Delta (tests/test_path_parity.py: test_path_parity_has_the_power_to_see_one_wrong_coefficient)."""
import numpy as np

from oracle import allegro_torch
from pair_allegro_amd import cg, model_file

import util

BAR = {"float32": 1e-4, "float64": 1e-10}        # max|Delta_kernel - Delta_oracle| <= BAR * max|Delta_oracle|, per quantity
DELTA_FRACTION = 0.1                             # b is the smallest boost with max|Delta F| >= DELTA_FRACTION * max|F(M+)|
BOOSTS = tuple(2.0 ** e for e in range(11))      # 1 .. 1024, capped: larger rows drive the activations towards float16's range (the f16x2 alarm)
QUANTITIES = ("forces", "eatom", "virial")
# ... plus two roundings of the quantity itself in the kernel's precision: the per-atom energies carry the shift (~5 eV), whose float32 ulp is ~5e-7
ROUNDING = {"float32": 2.0 * np.finfo(np.float32).eps, "float64": 2.0 * np.finfo(np.float64).eps}


def paths(cfg, layers=None):
    """[(layer k, path index p, (l1, l2, l3))] of every tensor product of the model; the last layer has the scalar paths only."""
    nl = cfg["num_layers"]
    return [(k, p, lll) for k in (layers or range(1, nl + 1)) for p, lll in enumerate(cg.tp_paths(cfg["l_max"], k == nl))]


def path_id(k, p, lll):
    return f"l{k}p{p}_{lll[0]}{lll[1]}{lll[2]}"


class PathCase:
    """One model on one geometry: the boost of every path (chosen on the float64 oracle), the oracle's Delta, the variant model files."""

    def __init__(self, model_dir, name, cfg, cell, pos, symbols, weights=None):
        self.cfg = dict(cfg)
        self.w = weights if weights is not None else model_file.init_weights(self.cfg)
        self.model_dir, self.name = model_dir, name
        self.cell, self.pos = np.asarray(cell, dtype=np.float64), np.asarray(pos, dtype=np.float64)
        self.names = sorted(set(symbols))
        self.types = np.array([self.names.index(s) + 1 for s in symbols], dtype=np.int32)
        self._boost = {}
        self._files = {}

    def weights(self, k, p, b):
        w = dict(self.w)
        tp = np.array(w[f"l{k}.tp"], dtype=np.float64)
        tp[p] *= b
        w[f"l{k}.tp"] = tp
        return w

    def oracle(self, w, edit_ctab=None):
        """float64 oracle evaluation; edit_ctab(ctab) may change the oracle's Clebsch-Gordan table in place first."""
        cfg64 = dict(self.cfg, model_dtype="float64")
        m = allegro_torch.build(cfg64, w)
        if edit_ctab is not None:
            import torch
            with torch.no_grad():
                edit_ctab(m.ctab)
        return util.oracle_run(cfg64, w, self.cell, self.pos, self.types, self.names, oracle=m)

    def oracle_delta(self, k, p, edit_ctab=None):
        b = self.boost(k, p)[0]
        plus, zero = self.oracle(self.weights(k, p, b), edit_ctab), self.oracle(self.weights(k, p, 0.0), edit_ctab)
        return {q: np.asarray(plus[q]) - np.asarray(zero[q]) for q in QUANTITIES}

    def boost(self, k, p):
        """(b, oracle Delta at b, max|q(M+)| per quantity): the smallest b of BOOSTS whose Delta is a sizeable part of the forces."""
        if (k, p) not in self._boost:
            zero = self.oracle(self.weights(k, p, 0.0))
            for b in BOOSTS:
                plus = self.oracle(self.weights(k, p, b))
                d = {q: np.asarray(plus[q]) - np.asarray(zero[q]) for q in QUANTITIES}
                frac = np.abs(d["forces"]).max() / np.abs(plus["forces"]).max()
                if frac >= DELTA_FRACTION:
                    break
            # a few paths feed the energy weakly (the l = 1 cross product (1, 1, 1) into the next layer's dot products): a quarter of it at the cap
            assert frac >= 0.25 * DELTA_FRACTION, f"path {k}/{p}: max|Delta F| / max|F| = {frac:.3g} at the largest boost {b}"
            self._boost[(k, p)] = (b, d, {q: np.abs(np.asarray(plus[q])).max() for q in QUANTITIES})
        return self._boost[(k, p)]

    def model_file(self, k, p, which, dtype):
        key = (k, p, which, dtype)
        if key not in self._files:
            b = self.boost(k, p)[0] if which == "plus" else 0.0
            path = f"{self.model_dir}/{self.name}_{dtype}_l{k}p{p}_{which}.ahip"
            model_file.save_ahip(path, dict(self.cfg, model_dtype=dtype), self.weights(k, p, b))
            self._files[key] = path
        return self._files[key]

    def kernel_delta(self, lib, k, p, dtype, options=None):
        plus = util.run_pair(lib, self.model_file(k, p, "plus", dtype), self.cell, self.pos, self.types, self.names, options=options)
        zero = util.run_pair(lib, self.model_file(k, p, "zero", dtype), self.cell, self.pos, self.types, self.names, options=options)
        assert plus["info"]["path"] == zero["info"]["path"], (plus["info"], zero["info"])
        for r in (plus, zero):
            for q in QUANTITIES:
                assert np.isfinite(r[q]).all(), (q, r["info"])
        return {q: plus[q] - zero[q] for q in QUANTITIES}, plus["info"]

    def check(self, lib, k, p, dtype, expect_path, options=None, bar=None):
        """Asserts the kernel's Delta against the oracle's on every quantity and the kernel path taken; returns the worst error / bar."""
        bar = BAR[dtype] if bar is None else bar
        _, ref, size = self.boost(k, p)
        got, info = self.kernel_delta(lib, k, p, dtype, options)
        assert info["path"] == expect_path, (info, expect_path)
        worst = 0.0
        for q in QUANTITIES:
            scale = np.abs(ref[q]).max()
            err = np.abs(got[q] - ref[q]).max()
            allowed = bar * scale + ROUNDING[dtype] * size[q]
            worst = max(worst, err / allowed)
            assert err <= allowed, (f"{self.name} layer {k} path {p} {cg.tp_paths(self.cfg['l_max'], k == self.cfg['num_layers'])[p]} "
                                        f"{info['path']}: {q} max|dDelta| {err:.3e} > {bar:g} * max|Delta| {scale:.3e} + rounding")
        return worst


def ctab_mutations(l1, l2, l3, p):
    """The three single-path mutations of the oracle's table the path-difference bar must see:
    the largest entry x 1.01, its sign flipped, two m3 components swapped (two m1 components for a scalar output; none for (0, 0, 0))."""
    c = cg.path_coeff(l1, l2, l3)
    idx = np.unravel_index(np.argmax(np.abs(c)), c.shape)

    def scale(t):
        t[(p,) + idx] *= 1.01

    def flip(t):
        t[(p,) + idx] *= -1.0

    def swap(t):
        if l3 > 0:
            a, b = t[p, :, :, 0].clone(), t[p, :, :, 2 * l3].clone()
            t[p, :, :, 0], t[p, :, :, 2 * l3] = b, a
        else:
            a, b = t[p, 0, :, :].clone(), t[p, 2 * l1, :, :].clone()
            t[p, 0, :, :], t[p, 2 * l1, :, :] = b, a

    out = [("x1.01", scale), ("sign", flip)]
    if l1 + l3 > 0:
        out.append(("swap", swap))
    return out


def oracle_edge_gradients(cfg, w, rs, lmp_names):
    """The float64 oracle's per-edge gradient dE/d(r_j - r_i) [E, 3] and its edge list [2, E] (atom indices of `rs`), in glue.preprocess order."""
    import torch
    from oracle import glue
    m = allegro_torch.build(dict(cfg, model_dtype="float64"), w)
    mapper, cm = util.type_mapper_and_cutoffs(cfg, lmp_names)
    inp = glue.preprocess(rs.x, rs.type, rs.nlocal, rs.ilist, rs.numneigh, rs.firstneigh, mapper, cm)
    pos, ei, ty = (torch.from_numpy(inp[k]) for k in ("pos", "edge_index", "atom_types"))
    rvec = (pos[ei[1]] - pos[ei[0]]).detach().requires_grad_(True)
    eps = m.edge_energy(rvec, ty[ei[0]], ty[ei[1]], ei[0], pos.shape[0])
    esum = torch.zeros(pos.shape[0], dtype=eps.dtype).index_add(0, ei[0], eps)
    ea = m.scale[ty] * (esum * m.inv_sqrt_nn) + m.shift[ty]
    return inp["edge_index"], torch.autograd.grad([ea.sum()], [rvec])[0].numpy()

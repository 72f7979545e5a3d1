"""Shared helpers of the parity tests (imports the oracle: tests only)."""
import hashlib
import json
import os

import numpy as np

from oracle import allegro_torch, glue
from pair_allegro_amd import lmp_like, model_file
from pair_allegro_amd.pair import PairAllegro, atom_from_rank_system, list_from_rank_system

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_TAGS = ["Si64_r5", "Cu-cubic_r5", "Cu-cubic_r15", "Cu2AgO4_r5", "aspirin_r5", "aspirin_r15", "CuPd-cubic-big_r5",
               "Li3PO4_128_r5", "water_192_r5",        # these two: samples of the BASELINE config 3 / 5 workloads (model S / model L)
               "Cu2AgO4_r5_l3", "Cu-cubic_r5_l3"]      # round 6: l_max = 3, widths off every fused shape (S 48, U 16, MLP 40, read-out 24): layer-at-a-time kernels

_model_cache = {}


def load_golden(tag):
    z = np.load(os.path.join(GOLDEN, tag + ".npz"))
    g = {k: z[k] for k in z.files}
    g["cfg"] = json.loads(str(g["cfg"]))
    g["symbols"] = [str(s) for s in g["symbols"]]
    g["lmp_type_names"] = [str(s) for s in g["lmp_type_names"]]
    g["tag"] = tag
    return g


def golden_model(g, model_dir, dtype):
    """Exports (once) the golden case's model as <tag>_<dtype>.nequip.pth; checks the weight hash."""
    key = (g["tag"], dtype)
    if key not in _model_cache:
        cfg = dict(g["cfg"])
        w = model_file.init_weights(cfg)
        assert hashlib.sha256(model_file.dumps(cfg, w)).hexdigest() == str(g["weights_sha256"]), \
            "seeded initialiser drifted from the golden fixtures"
        cfg["model_dtype"] = dtype
        path = os.path.join(model_dir, f"{g['tag']}_{dtype}.nequip.pth")
        allegro_torch.export_nequip_pth(path, cfg, w)
        _model_cache[key] = (path, cfg, w)
    return _model_cache[key]


def lammps_types(g):
    names = g["lmp_type_names"]
    return np.array([names.index(s) + 1 for s in g["symbols"]], dtype=np.int32), names


def run_pair(lib, model_path, cell, pos, types, lmp_names, skin=1.0, grid=(1, 1, 1), options=None, shuffle_seed=None):
    """The reference test's `run 0` on a px*py*pz rank grid: every rank builds its LAMMPS view,
    calls PairAllegro.compute, and the per-rank partial results are reduced the way LAMMPS does
    (ghost forces reverse-communicated to their owners, eng/virial summed over ranks)."""
    n = len(pos)
    forces = np.zeros((n, 3))
    eatom = np.zeros(n)
    pe = 0.0
    virial = np.zeros(6)
    edges = []
    info = {}
    ranks = lmp_like.grid_ranks(grid)
    for r in ranks:
        pair = PairAllegro(me=0, nprocs=1, lib=lib, quiet=True)
        pair.settings([])
        pair.coeff(["*", "*", model_path] + list(lmp_names), ntypes=len(lmp_names))
        for k, v in (options or {}).items():
            pair.model.set_option(k, v)
        pair.init_style()
        rs = lmp_like.build_rank_system(cell, pos, types, pair.init_one(1, 1) + skin, grid=grid, rank=r)
        if shuffle_seed is not None:                      # neighbour order must not matter
            rng = np.random.RandomState(shuffle_seed)
            for row in rs.firstneigh[: rs.nlocal]:
                rng.shuffle(row)
        atom = atom_from_rank_system(rs, len(lmp_names))
        pair.compute(atom, list_from_rank_system(rs))
        np.add.at(forces, rs.tag - 1, atom.f)
        if rs.nlocal:
            eatom[rs.tag[: rs.nlocal] - 1] = pair.eatom[: rs.nlocal]
        pe += pair.eng_vdwl
        virial += pair.virial
        if rs.nlocal:
            ei, rij = pair.model.get_edges()
            edges.append((rs.tag[ei[0]] - 1, rs.tag[ei[1]] - 1, rij))
            info["path"] = pair.model.last_path
            info["arith_note"] = pair.model.arith_note
            info["max_degree"] = max(info.get("max_degree", 0), pair.model.last_max_degree)
        pair.model.close()
    i = np.concatenate([e[0] for e in edges]); j = np.concatenate([e[1] for e in edges]); d = np.concatenate([e[2] for e in edges])
    return dict(forces=forces, eatom=eatom, pe=pe, virial=virial, edges=(i, j, d), info=info)


def type_mapper_and_cutoffs(cfg, lmp_names):
    """LAMMPS type -> model type index, and the [T][T] cutoff matrix over LAMMPS types (what the pair style hands the glue)."""
    model_types = cfg["type_names"]
    mapper = np.array([model_types.index(s) if s in model_types else -1 for s in lmp_names], dtype=np.int32)
    T = len(lmp_names)
    cm = np.full((T, T), cfg["r_max"])
    if cfg.get("per_edge_type_cutoff") is not None:
        pc = np.asarray(cfg["per_edge_type_cutoff"])
        for a in range(T):
            for b in range(T):
                cm[a, b] = pc[mapper[a], mapper[b]]
    return mapper, cm


def oracle_run(cfg, w, cell, pos, types, lmp_names, skin=1.0, oracle=None):
    """`oracle`: an already built (e.g. edited) allegro_torch module to evaluate instead of build(cfg, w)."""
    oracle = allegro_torch.build(cfg, w) if oracle is None else oracle
    rs = lmp_like.build_rank_system(cell, pos, types, cfg["r_max"] + skin)
    mapper, cm = type_mapper_and_cutoffs(cfg, lmp_names)
    f = np.zeros_like(rs.x)
    ea = np.zeros(rs.nall)
    eng, vir, inp = glue.compute(oracle, rs.x, rs.type, rs.nlocal, rs.ilist, rs.numneigh, rs.firstneigh, mapper, cm, f, ea)
    n = len(pos)
    forces = np.zeros((n, 3))
    np.add.at(forces, rs.tag - 1, f)
    eatom = np.zeros(n)
    eatom[rs.tag[: rs.nlocal] - 1] = ea[: rs.nlocal]
    return dict(forces=forces, eatom=eatom, pe=eng, virial=vir, inputs=inp, rs=rs)


def assert_close_to(res, ref, tol, stress_factor=20.0, what=""):
    """Reference tolerances: abs+rel tol on F, E_i, PE; x20 on the virial
    (/root/reference/tests/conftest.py:113, tests/test_python_repro_allegro.py:297-355)."""
    np.testing.assert_allclose(res["forces"], ref["forces"], atol=tol, rtol=tol, err_msg=f"forces {what}")
    np.testing.assert_allclose(res["eatom"], ref["eatom"], atol=tol, rtol=tol, err_msg=f"eatom {what}")
    np.testing.assert_allclose(res["pe"], float(ref["pe"]), atol=tol * max(1, len(ref["eatom"]) ** 0.5), rtol=tol, err_msg=f"pe {what}")
    np.testing.assert_allclose(res["eatom"].sum(), res["pe"], atol=1e-9 * max(1.0, abs(res["pe"])), rtol=1e-9, err_msg="PE != sum eatom")
    np.testing.assert_allclose(res["virial"], ref["virial"], atol=tol * stress_factor * max(1, len(ref["eatom"]) ** 0.5),
                               rtol=tol * stress_factor, err_msg=f"virial {what}")


# ---- TF32 emulation of the torch oracle (what `allow_tf32 = 1` licenses in the reference: /root/reference/pair_nequip_allegro.cpp:267-270) ----
class tf32_emulation:
    """Context manager: inside it every `a @ b` and every two-operand `torch.einsum` of an EAGER float32 module rounds both operands to
    TF32 (10 explicit mantissa bits, round to nearest even) before multiplying -- forward and, through a custom autograd function, the
    operand / gradient pairs of the backward matmuls -- and accumulates in float32: the arithmetic of a TF32 tensor-core run.  The
    three-operand tensor-product einsum stays float32 (fewer TF32 operations than a real run, i.e. a stricter bar for the kernel)."""

    @staticmethod
    def round_tf32(t):
        import torch
        if t.dtype != torch.float32:
            return t
        i = t.contiguous().view(torch.int32)
        lsb = (i >> 13) & 1
        i = (i + 0x0FFF + lsb) & ~0x1FFF
        return i.view(torch.float32)

    def __enter__(self):
        import torch
        r = tf32_emulation.round_tf32
        orig_mm, orig_es = torch.Tensor.__matmul__, torch.einsum
        self._orig = (orig_mm, orig_es)

        class _Contract(torch.autograd.Function):
            @staticmethod
            def forward(ctx, eq, a, b):
                ctx.eq = eq
                ctx.save_for_backward(a, b)
                return orig_es(eq, r(a), r(b)) if eq else orig_mm(r(a), r(b))

            @staticmethod
            def backward(ctx, g):
                a, b = ctx.saved_tensors
                with torch.enable_grad():
                    a_ = r(a).detach().requires_grad_(True)
                    b_ = r(b).detach().requires_grad_(True)
                    out = orig_es(ctx.eq, a_, b_) if ctx.eq else orig_mm(a_, b_)
                    ga, gb = torch.autograd.grad(out, [a_, b_], r(g.contiguous()))
                return None, ga, gb

        def mm(a, b):
            return _Contract.apply("", a, b) if a.dtype == torch.float32 else orig_mm(a, b)

        def es(eq, *ops):
            if len(ops) == 2 and ops[0].dtype == torch.float32:
                return _Contract.apply(eq, ops[0], ops[1])
            return orig_es(eq, *ops)

        torch.Tensor.__matmul__ = mm
        torch.einsum = es
        return self

    def __exit__(self, *exc):
        import torch
        torch.Tensor.__matmul__, torch.einsum = self._orig
        return False


# ---- the split arithmetics of k_fused, emulated on the torch oracle (csrc/fused_h.h, csrc/fused.hip: linear_b) ----
class split_emulation:
    """Context manager: inside it every `a @ b` and every two-operand `torch.einsum` of an EAGER float32 module is evaluated the way the fused
    kernel's linears evaluate it, forward and (through a custom autograd function) backward, with float32 accumulation:
      "f16x2"  -- v = hi + 2^-11 lo', hi = f16(v), lo' = f16((v - hi) 2^11), both round-to-nearest; product = hi hi + 2^-11 (hi lo' + lo' hi)
      "bf16x3" -- v = hi + mid + lo by truncation to bf16; the six products of weight >= 2^-16
      "f32"    -- nothing changed (the yardstick)
    What this pins on the CPU is the claim that the splits are float32-EQUIVALENT for the model: same distance from the float64 oracle."""

    def __init__(self, mode):
        assert mode in ("f32", "f16x2", "bf16x3")
        self.mode = mode

    @staticmethod
    def f16_terms(t):
        import torch
        hi = t.to(torch.float16).to(torch.float32)
        lo = ((t - hi) * 2048.0).to(torch.float16).to(torch.float32) / 2048.0
        return hi, lo

    @staticmethod
    def bf16_terms(t):
        import torch
        tr = lambda q: (q.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32)
        hi = tr(t); r = t - hi; mid = tr(r); lo = tr(r - mid)
        return hi, mid, lo

    def contract(self, f, a, b):
        if self.mode == "f16x2":
            ah, al = self.f16_terms(a); bh, bl = self.f16_terms(b)
            return f(ah, bh) + (f(ah, bl) + f(al, bh))
        if self.mode == "bf16x3":
            a0, a1, a2 = self.bf16_terms(a); b0, b1, b2 = self.bf16_terms(b)
            return ((f(a2, b0) + f(a1, b1) + f(a0, b2)) + (f(a1, b0) + f(a0, b1))) + f(a0, b0)
        return f(a, b)

    def __enter__(self):
        import torch
        orig_mm, orig_es = torch.Tensor.__matmul__, torch.einsum
        self._orig = (orig_mm, orig_es)
        me = self

        class _Contract(torch.autograd.Function):
            @staticmethod
            def forward(ctx, eq, a, b):
                ctx.eq = eq
                ctx.save_for_backward(a, b)
                return me.contract((lambda x, y: orig_es(eq, x, y)) if eq else orig_mm, a, b)

            @staticmethod
            def backward(ctx, g):
                a, b = ctx.saved_tensors
                g = g.contiguous()

                def vjp(wrt_a):          # (gradient term, other-operand term) -> the contraction that yields the gradient w.r.t. one operand
                    def f(gt, ot):
                        v = (a if wrt_a else b).detach().clone().requires_grad_(True)
                        with torch.enable_grad():
                            out = (orig_es(ctx.eq, v, ot) if wrt_a else orig_es(ctx.eq, ot, v)) if ctx.eq else (orig_mm(v, ot) if wrt_a else orig_mm(ot, v))
                        return torch.autograd.grad(out, v, gt)[0]
                    return f
                return None, me.contract(vjp(True), g, b), me.contract(vjp(False), g, a)

        def mm(a, b):
            return _Contract.apply("", a, b) if a.dtype == torch.float32 else orig_mm(a, b)

        def es(eq, *ops):
            if len(ops) == 2 and ops[0].dtype == torch.float32:
                return _Contract.apply(eq, ops[0], ops[1])
            return orig_es(eq, *ops)

        torch.Tensor.__matmul__ = mm
        torch.einsum = es
        return self

    def __exit__(self, *exc):
        import torch
        torch.Tensor.__matmul__, torch.einsum = self._orig
        return False

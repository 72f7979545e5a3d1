"""The instance table of the fused kernels (csrc/fused_shapes.h: FUSED_INSTANCES) against everything that has to agree with it, on the CPU:
  * the kernel instances each object really compiles: every (source, part) of the table is compiled host-only and its k_fused / k_fused_lx / k_fused_lx2 symbols are
    compared, as sets and per object, with the table enumerated to full template argument lists by a stand-alone g++ program;
  * csrc/Makefile: every row's object is built from the row's source with the row's part define, and the fused objects of OBJS are the table's;
  * the lookups fused_instance_exists / fused_has_wide_tile against the boolean cascades they replaced, kept here verbatim as Python, over the whole grid;
  * dispatch<Choices<...>>: a run-time value that is in none of the choices is a StateError, not the last choice."""
import concurrent.futures
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pair_allegro_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

DUMP_MAIN = r"""
#include <cstdio>
#include <cstring>
#include "fused_shapes.h"
using namespace ahip;
static const char *B(bool b) { return b ? "true" : "false"; }
int main(int argc, char **argv) {
  if (argc == 2 && !std::strcmp(argv[1], "instances")) {
    // <object> <source> <part> <kernel<template arguments as nm -C prints them>>
    for (const FusedInstanceRow &r : FUSED_INSTANCES)
      for (int ar = 0; ar < 4; ++ar)
        for (int tb = 0; tb < 2; ++tb)
          for (int md = 0; md < 8; ++md)
            for (int tile = 1; tile < 16; ++tile)
              for (int nl = 1; nl < 8; ++nl)
                for (int var = 0; var < 3; ++var) {
                  if (r.family != FusedFamily::k_fused && tb == 0) continue;      // the wide kernels have no two-body template parameter
                  if (fused_find_instance({r.family, ar, tb != 0, md, r.RD, r.WF, r.RF, true, tile, nl, var}) != &r) continue;
                  if (!fi_has(r.ar, ar)) return 3;
                  std::printf("%s %s %d ", r.object, r.source, r.part);
                  const char *prof = B(var == VAR_PROF), *va = B(var == VAR_VA);
                  if (r.family == FusedFamily::k_fused)
                    std::printf("k_fused<%d, %s, %d, %s, %d, %d, %s, %d, %d, %d>\n", tile, prof, ar, B(tb != 0), nl, md, va, r.RD, r.WF / 16, r.RF / 16);
                  else if (r.family == FusedFamily::lx32)
                    std::printf("k_fused_lx<%d, %d, %s, %d, %s, %d, %d, %d, %d>\n", tile, nl, prof, ar, va, md, r.RD, r.WF / 16, r.RF / 16);
                  else
                    std::printf("k_fused_lx2<%d, %s, %d, %s, %d, %d, %d, %d>\n", nl, prof, ar, va, md, r.RD, r.RF / 16, r.WF / 32);
                }
    return 0;
  }
  if (argc == 2 && !std::strcmp(argv[1], "lookups")) {
    // family arith tb MD RD WF RF lx64_w128 -> exists, wide tile; then the five words of option fused_arith resolved as the C-ABI resolves them
    const FusedFamily fams[] = {FusedFamily::none, FusedFamily::k_fused, FusedFamily::lx32, FusedFamily::lx64};
    const ArithOpt opts[] = {ArithOpt::Auto, ArithOpt::F32, ArithOpt::F16x2, ArithOpt::Bf16x3, ArithOpt::Tf32eq};
    for (FusedFamily f : fams)
      for (int a = 0; a < 4 + 5; ++a)
        for (int tb = 0; tb < 2; ++tb)
          for (int md = 0; md <= 4; ++md)
            for (int rd = 0; rd <= 3; ++rd)
              for (int WF : {64, 128})
                for (int RF : {32, 64})
                  for (int w = 0; w < 2; ++w) {
                    const Arith ar = a < 4 ? (Arith)a : resolve_arith(opts[a - 4], false, false, false, tb != 0, fused_is_wide(f));
                    std::printf("%s %d %d %d %d %d %d %d %d %d\n", fused_family_name(f), (int)ar, tb, md, rd, WF, RF, w,
                                (int)fused_instance_exists(f, ar, tb != 0, md, rd, WF, RF, w != 0), (int)fused_has_wide_tile(f, ar, md, rd, WF, RF));
                  }
    return 0;
  }
  if (argc == 2 && !std::strcmp(argv[1], "dispatch")) {
    int got = 0;
    dispatch<Choices<4, 8>>([&](auto nw) { got = nw; }, 8);
    if (got != 8) return 3;
    dispatch<Choices<4, 8>, Choices<1, 2, 3>>([&](auto nw, auto nl) { got = 10 * nw + nl; }, 4, 3);
    if (got != 43) return 3;
    try {
      dispatch<Choices<4, 8>>([&](auto nw) { got = nw; }, 5);
    } catch (const StateError &e) {
      std::printf("StateError: %s\n", e.what());
      return got == 43 ? 0 : 3;
    }
    return 4;      // ran on some choice
  }
  return 2;
}
"""


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("instance_table")
    src, exe = d / "dump_main.cpp", d / "dump_main"
    src.write_text(DUMP_MAIN)
    # plain host compiler, no HIP include path: the header must stand on its own
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), os.path.join(CSRC, "model_io.cpp"), "-o", str(exe)], check=True)
    return lambda what: subprocess.run([str(exe), what], check=True, stdout=subprocess.PIPE).stdout.decode().splitlines()


@pytest.fixture(scope="module")
def table(dump):
    """{object: (source, part, {kernel<arguments>})}"""
    out = {}
    for ln in dump("instances"):
        obj, source, part, inst = ln.split(" ", 3)
        src, prt, insts = out.setdefault(obj, (source, int(part), set()))
        assert (src, prt) == (source, int(part)), "one (source, part) per object"
        assert inst not in insts, ("two rows name one instance", inst)
        insts.add(inst)
    return out


@pytest.fixture(scope="module")
def make_lines():
    """{object: the compile command `make` would run for it}"""
    objs = re.search(r"^OBJS\s*=(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    out = {}
    for o in objs:
        if not o.startswith("fused"):
            continue
        lines = subprocess.run(["make", "-n", "-B", "-C", CSRC, o], check=True, stdout=subprocess.PIPE).stdout.decode().splitlines()
        cmd = [ln for ln in lines if " -c " in ln and ("-o " + o) in ln]
        assert len(cmd) == 1, (o, lines)
        out[o[:-2]] = cmd[0].split()
    return out


def _part_define(source):
    return "-DAHIP_FUSED_PART=" if source == "fused.hip" else "-DAHIP_LX_PART="


def test_table_equals_makefile(table, make_lines):
    assert set(make_lines) == set(table), "the fused objects of OBJS are the objects of the table"
    assert len({(s, p) for s, p, _ in table.values()}) == len(table), "one object per (source, part)"
    for obj, (source, part, _) in table.items():
        words = make_lines[obj]
        assert source in words, (obj, words)
        parts = [w for w in words if w.startswith(_part_define(source))]
        # (a source compiled without its part define is part 0: the #ifndef at the head of its host side)
        assert parts == [_part_define(source) + str(part)] or (part == 0 and not parts), (obj, parts)


def test_table_equals_compiled_instances(table, make_lines, tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc: the objects' instances cannot be enumerated")

    def compiled(obj):
        source = table[obj][0]
        defines = [w for w in make_lines[obj] if w.startswith("-DAHIP_")]      # the part, and AHIP_NO_ACC_PARK where the Makefile gives it
        o = str(tmp_path / (obj + ".o"))
        subprocess.run([HIPCC, "--cuda-host-only", "-O1", "-std=c++17", "-c"] + defines + [os.path.join(CSRC, source), "-o", o], check=True, cwd=CSRC)
        syms = subprocess.run(["nm", "-C", o], check=True, stdout=subprocess.PIPE).stdout.decode()
        return set(re.findall(r"\b(k_fused(?:_lx2?)?<[^<>]*>)\(", syms))

    with concurrent.futures.ThreadPoolExecutor(4) as pool:
        got = dict(zip(table, pool.map(compiled, table)))
    for obj, (_, _, want) in table.items():
        assert got[obj] == want, (obj, "compiled, not in the table:", sorted(got[obj] - want), "in the table, not compiled:", sorted(want - got[obj]))
    print("instances per object:", {o: len(v) for o, v in got.items()}, "total", sum(len(v) for v in got.values()))


AR_F32, AR_BF16X3, AR_TF32EQ, AR_F16X2 = 0, 1, 2, 3
FUSED_WF, FUSED_WF2, FUSED_RF, FUSED_RF2 = 64, 128, 32, 64


def _is_wide(f):
    return f in ("lx32", "lx64")


def _old_instance_exists(f, ar, tb_table, MD, RD, WF, RF, lx64_w128):
    """fused_instance_exists as it was before the table, line by line."""
    if f == "none" or MD < 1 or MD > 3 or RD < 1 or RD > 2:
        return False
    if RF == FUSED_RF2:
        return WF == FUSED_WF and ar == AR_F16X2 and RD == 1 and (_is_wide(f) or tb_table)
    if RF != FUSED_RF:
        return False
    if WF == FUSED_WF2:
        return (f == "k_fused" or f == "lx32" or (f == "lx64" and lx64_w128)) and ar == AR_F16X2 and RD == 1 and (_is_wide(f) or tb_table)
    if WF != FUSED_WF:
        return False
    if MD == 2 and RD == 1:
        return (ar == AR_F32 or ar == AR_F16X2) if _is_wide(f) else (ar != AR_F16X2 or tb_table)
    return ar == AR_F16X2 and (_is_wide(f) or tb_table)


def _old_has_wide_tile(f, ar, MD, RD, WF, RF):
    """fused_has_wide_tile as it was before the table."""
    return f == "lx32" and (ar == AR_F32 or ar == AR_F16X2) and MD == 2 and RD == 1 and WF == FUSED_WF and RF == FUSED_RF


def test_lookups_equal_the_old_rule(dump):
    """family (and none) x the 4 arithmetics the kernels have and the 5 words of option fused_arith as they resolve x two-body mode x MD 0..4 x RD 0..3 x WF x RF x lx64_w128"""
    lines = dump("lookups")
    assert len(lines) == 4 * 9 * 2 * 5 * 4 * 2 * 2 * 2
    diffs = []
    for ln in lines:
        f, *v = ln.split()
        ar, tb, md, rd, WF, RF, w, exists, wide = (int(x) for x in v)
        want = (int(_old_instance_exists(f, ar, bool(tb), md, rd, WF, RF, bool(w))), int(_old_has_wide_tile(f, ar, md, rd, WF, RF)))
        if (exists, wide) != want:
            diffs.append((ln, want))
    assert not diffs, diffs[:10]
    assert sum(int(ln.split()[-2]) for ln in lines) > 0 and sum(int(ln.split()[-1]) for ln in lines) > 0


def test_dispatch_refuses_a_value_that_is_none_of_its_choices(dump):
    assert dump("dispatch")[0].startswith("StateError: instance dispatch: 5 ")

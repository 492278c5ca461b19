"""CPU tests of the drop-in boundary: the C-ABI library loads without a GPU, exports every symbol the header declares,
fails loudly (never falls back to a CPU path) when there is no device, and the host-only entry points work."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols(header="arkblst_amd.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported(pkg):
    L = pkg.load_library()
    syms = _declared_symbols()
    assert len(syms) >= 16
    for s in syms:
        assert hasattr(L, s), f"{s} declared in include/arkblst_amd.h but not exported"


def test_rccl_header_symbols_are_exported(pkg):
    """include/arkblst_amd_rccl.h against libarkblst_amd_rccl.so: every declared entry point is exported, the RCCL calls are IMPORTED
    (the library, not a Python host, issues the collective), and the product library itself does not pull RCCL in."""
    import subprocess

    L = pkg.load_rccl_library()
    syms = _declared_symbols("arkblst_amd_rccl.h")
    assert len(syms) >= 9 and "mi_msm_g1_allgather_fold" in syms and "mi_msm_g2_allgather_fold" in syms
    for s in syms:
        assert hasattr(L, s), f"{s} declared in include/arkblst_amd_rccl.h but not exported"
    und = subprocess.check_output(["nm", "-D", "--undefined-only", pkg.rccl_lib_path()]).decode()
    for s in ("ncclAllGather", "ncclCommInitRank", "ncclGetUniqueId", "mi_msm_g1_device_windows", "mi_g1_fold_windows"):
        assert s in und, s
    needed = subprocess.check_output(["readelf", "-d", pkg.rccl_lib_path()]).decode()
    assert "librccl.so.1" in needed and "libarkblst_amd.so" in needed
    assert "rccl" not in subprocess.check_output(["readelf", "-d", pkg.lib_path()]).decode()


def _exported(path):
    import subprocess

    out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_product_library_has_no_test_hooks(pkg):
    """mi_test_* entry points exist only in the test build (csrc/test_hooks.h); the product exports exactly the header"""
    prod = {s for s in _exported(pkg.lib_path()) if s.startswith("mi_")}
    assert prod == set(_declared_symbols()), prod ^ set(_declared_symbols())
    test = {s for s in _exported(pkg.lib_path(True)) if s.startswith("mi_")}
    assert test - prod == {"mi_test_fp_op", "mi_test_field_op", "mi_test_field_op_info", "mi_test_set_pairing", "mi_test_set_max_part", "mi_test_fail_allocs", "mi_test_plan",
                           "mi_test_set_no_peer", "mi_test_pairing_stage"}
    # ... and the plan switches of the test build (csrc/msm_sort.hip reads them from the environment): their names are in its image only
    image = {t: open(pkg.lib_path(t), "rb").read() for t in (False, True)}
    for name in (b"MI_TEST_SERIAL_MIN_BUCKETS", b"MI_TEST_SERIAL_L", b"MI_TEST_COOP_L"):
        assert name in image[True] and name not in image[False], name
    assert b"MI_TEST_" not in image[False]


def test_hot_kernels_do_not_spill(pkg):
    """Reads the gfx950 code objects inside the SHIPPED library (what `llvm-readelf --notes` prints) and fails when a hot kernel
    — accumulate, reduce, combine, the Miller kernels, the Fp12 tree — reports spilled registers: round 2 shipped a G2 accumulate
    loop with 35 spilled VGPRs (2.8 GB of scratch writes per launch) under a comment that said it ran without scratch."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    res = kr.resources(pkg.lib_path())
    hot = {k: v for k, v in res.items() if kr.is_hot(k)}
    assert len(hot) >= 9, sorted(hot)
    for want in ("k_accumulate<msmk::G1C>", "k_accumulate_g2_coop", "k_reduce_serial", "k_reduce_coop<msmk::QuadG1>", "k_miller_accumulate",
                 "k_miller_lines2", "k_fp12_prod"):
        assert any(want in k for k in hot), want
    spilling = {k: (v["vgpr_spill_count"], v["sgpr_spill_count"]) for k, v in hot.items()
                if v.get("vgpr_spill_count", 0) or v.get("sgpr_spill_count", 0)}
    assert not spilling, spilling
    # ... and no scratch traffic inside their arithmetic loops at all (an address-taken loop variable lives in scratch without
    # counting as a spill: read off the disassembly)
    loops = kr.scratch_in_hot_loops(pkg.lib_path())
    assert len(loops) >= 9 and not {k: v for k, v in loops.items() if v}, loops
    # two waves per SIMD where the design says so: at most 256 registers (VGPR + AGPR share one 512-entry file per SIMD lane)
    for k, v in hot.items():
        if "k_reduce_coop<msmk::PairG2>" in k or "k_fp12_prod" in k or "k_miller_accumulate" in k:
            continue   # one wave per SIMD by design (DESIGN_HISTORY.md §2.6; the pairing's accumulate / tree kernels keep three column sets)
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= 256, (k, v)


def test_no_kernel_mixes_calls_and_agprs(pkg):
    """Guard for the compiler issue of round 4 (csrc/Makefile, DESIGN_HISTORY.md §9 "call-ABI miscompare"; reproducer
    tools/call_abi/repro_tower.hip): ROCm 7.2's hipcc miscompiles a kernel that keeps values across calls of out-of-line device
    functions when interprocedural register allocation meets VGPR spills into AGPRs.  The library never lets the two meet: a
    kernel with a call in its body is built for <= 256 registers per lane (.agpr_count, which the assembler maximises over the
    callees, is 0), a kernel that uses AGPRs contains no call.  Read off the shipped code objects of BOTH builds."""
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import kernel_resources as kr

    for test_hooks in (False, True):
        lib = pkg.lib_path(test_hooks)
        res, calls = kr.resources(lib), kr.kernels_with_calls(lib)
        assert len(res) > 60 and set(res) == set(calls)
        mixed = {k: (v["vgpr_count"], v["agpr_count"]) for k, v in res.items() if calls[k] and v.get("agpr_count", 0) > 0}
        assert not mixed, mixed
        assert any(calls.values()) and any(v.get("agpr_count", 0) > 0 for v in res.values())   # both kinds exist: the check is not vacuous


def test_layout_sizes_match_reference_types(pkg):
    # blst_p1_affine 96, blst_p1 144, blst_p2_affine 192, blst_p2 288 (src/gpu.rs:69-71)
    from ark_blst_amd import binding as b

    assert (b.G1_AFF, b.G1_JAC, b.G2_AFF, b.G2_JAC) == (96, 144, 192, 288)
    assert C.sizeof(b.Profile) == 11 * 8 + 2 * 4 + 2 * 8 + 4 * 4 + 3 * 8   # mi_profile (round 6: + window_groups, reserved, the in-kernel clock)


def test_strerror_and_invalid_args(pkg):
    L = pkg.load_library()
    assert L.mi_msm_strerror(0) == b"ok"
    assert L.mi_msm_strerror(-2) == b"no usable HIP device"
    assert L.mi_msm_init(None, None, 1) == -1  # MI_E_INVALID


def test_no_device_fails_loudly(pkg):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(pkg.MsmError) as e:
        pkg.Context([0])
    assert e.value.code == -2  # MI_E_NO_DEVICE: no silent CPU path


def test_host_fold_of_partials_matches_oracle(pkg, co, o):
    """mi_g1_sum / mi_g2_sum: the deterministic fold that follows the all-gather of per-GPU partial sums."""
    for group, F, gen in (("g1", o.F1, o.G1_GEN), ("g2", o.F2, o.G2_GEN)):
        ks = [5, 7, 11, 0, 123456789]
        parts = [o.jac_to_bytes(F, o.scalar_mul(F, gen, k)) for k in ks]
        # add a non-trivially scaled Jacobian representative: use the C oracle's Pippenger output as one partial
        aff = 96 if group == "g1" else 192
        bases = co.gen_bases(group, 5, 8, 1)
        sc = co.gen_scalars(6, 8)
        parts.append(co.msm(group, bases, sc, 8, 0, 1))
        got = (pkg.g1_sum if group == "g1" else pkg.g2_sum)(parts)
        want = co.sum_jac(group, b"".join(parts), len(parts))
        assert co.to_affine(group, got) == co.to_affine(group, want)
        # P + P (doubling inside the fold) and P + (-P)
        p = parts[1]
        dbl = (pkg.g1_sum if group == "g1" else pkg.g2_sum)([p, p])
        assert co.to_affine(group, dbl) == o.affine_to_bytes(F, o.scalar_mul(F, gen, 14))
        assert len(got) == (144 if group == "g1" else 288) and aff


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_fold_windows_host(pkg, co, o, group):
    """mi_g{1,2}_fold_windows (host only): the tail of the multi-process exchange — per-window sums of several ranks, added in
    rank order per window, then Horner over the windows.  Expected value from the Python big-int oracle: the points are known
    multiples k[r][w] G, so the fold is (sum_w 2^(c w) sum_r k[r][w]) G."""
    import random

    F, gen = (o.F1, o.G1_GEN) if group == "g1" else (o.F2, o.G2_GEN)
    size = 144 if group == "g1" else 288
    rnd = random.Random(77)
    for ranks, nwin, c, stride in ((1, 1, 16, 1), (3, 5, 7, 5), (2, 13, 20, 37), (8, 16, 16, 16), (4, 37, 7, 37)):
        k = [[rnd.randrange(0, 1 << 64) for _ in range(nwin)] for _ in range(ranks)]
        k[0][0] = 0                                        # a window sum at infinity
        if ranks > 1 and nwin > 1:
            k[1][1] = o.R_ORDER - k[0][1]                  # two ranks cancel in one window
        blob = bytearray(ranks * stride * size)
        for r in range(ranks):
            for w in range(nwin):
                pt = o.scalar_mul(F, gen, k[r][w])
                blob[(r * stride + w) * size:(r * stride + w + 1) * size] = o.jac_to_bytes(F, o.jac_from_aff(F, pt)) if pt is not o.INF else bytes(size)
        got = pkg.fold_windows(group, bytes(blob), ranks, stride, c, nwin)
        total = sum((1 << (c * w)) * sum(k[r][w] for r in range(ranks)) for w in range(nwin)) % o.R_ORDER
        want = o.scalar_mul(F, gen, total)
        assert co.to_affine(group, got) == (o.affine_to_bytes(F, want) if want is not o.INF else bytes(2 * size // 3)), (ranks, nwin, c)
    # argument checks: more windows than MI_MAX_WINDOWS, a stride shorter than the window count
    import ctypes as C2
    from ark_blst_amd import binding as b

    L = pkg.load_library()
    out = C2.create_string_buffer(size)
    assert getattr(L, f"mi_{group}_fold_windows")(bytes(size * 40), 1, 40, C2.byref(b.WindowInfo(16, 38)), out) == -1
    assert getattr(L, f"mi_{group}_fold_windows")(bytes(size * 4), 1, 2, C2.byref(b.WindowInfo(16, 4)), out) == -1
    assert getattr(L, f"mi_{group}_fold_windows")(None, 0, 0, C2.byref(b.WindowInfo(0, 0)), out) == 0 and out.raw == bytes(size)


def test_reference_style_length_mismatch_error(pkg):
    """VariableBaseMSM::msm returns Err(min(len)) on a length mismatch (arkworks default)."""
    with pytest.raises(pkg.msm.MsmErr) as e:
        pkg.G1Projective.msm(bytes(96 * 3), bytes(32 * 2))
    assert e.value.value == 2


def test_plan_geometry_invariants(pkg):
    """The window-size plan (make_plan: the role of calc_window_size / calc_chunk_size, /root/reference/src/gpu.rs:64-92,218-223) over
    sizes from 1 point to the 2^26 per-pass limit, free and forced window sizes, both groups, plain and shared bucket sets: the
    geometry every kernel launch relies on (32-bit entry offsets, index + sign + fine bits in one word, coarse bins within the
    LDS counter array, power-of-two chunks inside a window, staged-sort limits)."""
    import random

    rnd = random.Random(5)
    sizes = [1, 2, 63, 64, 65, 1000, 4095, 4096, 4097] + [1 << k for k in range(10, 27)] + [(1 << k) - 12345 for k in (20, 21, 24, 26)] + \
            [rnd.randrange(1, 1 << 26) for _ in range(40)]
    for group in ("g1", "g2"):
        for n in sizes:
            for shared, fold in ((False, False), (True, False), (False, True), (True, True)):
                for c in [0] + list(range(7, 23)):
                    stride = n if shared else 0
                    p = pkg.test_plan(n, c, group, shared, stride, fold)
                    if p["c"] == 0:
                        assert c != 0 or shared, (group, n, "the free plan must exist for every size")   # a forced c may not fit the geometry
                        continue
                    cc = p["c"]
                    assert 7 <= cc <= 22 and (c == 0 or cc == c)
                    # the integer s < r < 2^255 is recoded: a full top window (c | 255) can carry into one more; a validated set recodes min(s, r - s) < 2^254
                    assert p["nwin"] == (255 + cc - 1) // cc + (1 if 255 % cc == 0 and not fold else 0) and p["bwin"] == (1 if shared else p["nwin"])
                    assert p["nwin"] <= 37                                                     # MI_MAX_WINDOWS
                    assert n * p["nwin"] < 1 << 32                                            # entry offsets are 32-bit
                    nb = 1 << (cc - 1)
                    assert p["nbuckets"] == nb * p["bwin"]
                    idx_bits = max(1, ((max(stride, n) * p["nwin"]) if shared else n) - 1).bit_length()
                    assert idx_bits + 1 + p["lo_bits"] <= 32 and p["lo_bits"] <= min(8, cc - 1)   # index | sign | fine bits in one word
                    assert (nb >> p["lo_bits"]) <= 16384                                      # coarse bins of a window fit the LDS counters
                    assert p["nchunks"] == p["chunks_per_win"] * p["bwin"]
                    assert 5 <= p["logT"] <= 20
                    if p["serial"]:   # one lane per serial_L buckets of a window (any L <= 64), ragged last lane
                        assert group == "g1" and p["nbuckets"] >= 1 << 21 and 8 <= p["serial_L"] <= 64
                        assert p["chunks_per_win"] == -(-nb // p["serial_L"])
                    else:
                        # one wave per chunk_buckets = NLL x coop_L buckets (any L <= 64), ragged last chunk of a window
                        assert p["chunk_buckets"] <= nb and p["chunks_per_win"] == -(-nb // p["chunk_buckets"]) and p["serial_L"] == 0
                        assert p["chunk_buckets"] == p["coop_L"] * (16 if group == "g1" else 32) and 1 <= p["coop_L"] <= 64
    # no window size fits the entry encoding of precomputed tables beyond ~9e7 points per device (n x windows > 2^30 entries): the plan
    # says so (c = 0) and mi_msm_g1_set_bases_precomputed turns that into MI_E_INVALID before it divides by c
    assert pkg.test_plan(100_000_000, 0, "g1", True, 100_000_000)["c"] == 0
    # the sizes the benchmark configs use keep their measured choices
    # (round 4: with the scalar's sign folded into the digits c = 17 needs 15 windows, not 16, and wins from 2^22 up: 21.5 vs 22.1 ms at 2^23;
    #  round 5: the fold is the plan of a VALIDATED resident set only — the plain plan recodes the integer and c = 15 / 17 carry an extra window)
    vp = lambda n, *a: pkg.test_plan(n, *a, fold=True)
    assert vp(1 << 20)["c"] == 16 and vp(1 << 21)["c"] == 17 and vp(1 << 23)["c"] == 17   # 2^21: 5.71 (17) vs 6.02 ms (16)
    assert vp(1 << 23)["nwin"] == 15 and vp(1 << 16)["c"] == 15
    assert pkg.test_plan(1 << 21)["c"] == 16 and pkg.test_plan(1 << 16, 15)["nwin"] == 18 and pkg.test_plan(1 << 21, 17)["nwin"] == 16
    assert pkg.test_plan(1 << 24)["c"] == 20 and pkg.test_plan(1 << 24)["serial"] == 1 and pkg.test_plan(1 << 24)["serial_L"] == 53
    assert pkg.test_plan(1 << 20, 0, "g2")["c"] == 16
    # the reduce wave's L is not tied to powers of two: 17 windows of 2^14 buckets fit one round of wave slots at L = 9
    assert vp(1 << 16, 15)["coop_L"] == 9 and vp(1 << 16, 15)["nchunks"] == 17 * 114
    assert pkg.test_plan(1 << 20)["coop_L"] == 16 and pkg.test_plan(1 << 20)["nchunks"] == 2048


def test_plan_picks_against_the_committed_scans(pkg):
    """The plan's window size against the forced-c scans taken on MI355X after the last change of the pipeline
    (profiles/r04_scan_c_*_merge_tree.jsonl, *_final.jsonl: every window size forced at 2^8 .. 2^24 points, both groups): at every
    scanned size the plan's choice must have measured within 15 % of the best choice (the two known misses are G2 2^13 / 2^14 at
    13 %, DESIGN_HISTORY.md section 9).  Host only: the plan needs no device."""
    import glob
    import json

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = sorted(glob.glob(os.path.join(root, "profiles", "r04_scan_c_*_merge_tree.jsonl")) +
                   glob.glob(os.path.join(root, "profiles", "r04_scan_c_*_final.jsonl")))
    assert files
    tab = {}
    for f in files:
        for line in open(f):
            r = json.loads(line)
            if r["forced_c"] and r["ok"]:
                t = tab.setdefault((r["group"], r["log_n"]), {})
                t[r["forced_c"]] = min(t.get(r["forced_c"], 1e9), r["ms"])
    checked = 0
    for (group, log_n), t in sorted(tab.items()):
        c = pkg.test_plan(1 << log_n, 0, group, fold=True)["c"]   # the round-4 scans ran with the sign fold
        if c not in t:
            continue   # the scan did not force this window size
        assert t[c] <= 1.15 * min(t.values()), (group, log_n, c, t)
        checked += 1
    assert checked >= 25
    # round 5: the PLAIN plan (integer recoding: what every unvalidated base set gets) against its own scan, 2^10 .. 2^23 points
    # ... and the round-5 scans of both plans, G1 and G2 (the validated plan folds the scalars' signs)
    for kind, fold in (("plain", False), ("validated", True)):
        tab = {}
        for f in sorted(glob.glob(os.path.join(root, "profiles", f"r05_scan_c_*_{kind}.jsonl"))):
            for line in open(f):
                r = json.loads(line)
                if r["forced_c"] and r["ok"] and bool(r.get("validated")) == fold:
                    t = tab.setdefault((r["group"], r["log_n"]), {})
                    t[r["forced_c"]] = min(t.get(r["forced_c"], 1e9), r["ms"])
        assert len(tab) >= 15, kind
        for (group, log_n), t in sorted(tab.items()):
            c = pkg.test_plan(1 << log_n, 0, group, fold=fold)["c"]
            assert c in t and t[c] <= 1.15 * min(t.values()), (kind, group, log_n, c, t)


def test_binding_refuses_the_wrong_load_order():
    """the library loaded BEFORE torch leaves the process with two HIP runtimes and torch without devices; the binding says so
    when the first context is created instead of letting 'No HIP GPUs are available' surface somewhere else.  The right order passes."""
    import subprocess
    import sys

    prog = """
import sys
sys.path.insert(0, %r)
import __graft_entry__ as g
g.load_package()
from ark_blst_amd import binding as b
ORDER
try:
    b.check_runtime_order()
    print("accepted")
except ImportError as e:
    print("refused", "TWO HIP runtimes" in str(e))
""" % ROOT
    bad = subprocess.run([sys.executable, "-c", prog.replace("ORDER", "b.load_library()\nimport torch")], capture_output=True, text=True, timeout=600)
    good = subprocess.run([sys.executable, "-c", prog.replace("ORDER", "import torch\nb.load_library()")], capture_output=True, text=True, timeout=600)
    assert bad.stdout.strip().endswith("refused True"), bad.stdout + bad.stderr[-2000:]
    assert good.stdout.strip().endswith("accepted"), good.stdout + good.stderr[-2000:]


def test_kernels_that_run_beside_the_accumulate_kernel_fit_there(pkg):
    """Round 6: k_accumulate<G1C> holds two waves of 216 registers on every SIMD, so a workgroup is dispatched beside it only
    when its waves need at most 80 registers per lane and SIMD — counted in what the hardware ALLOCATES (the kernel descriptor), which the compiler
    pads for kernels with large static LDS.  The sort and schedule kernels of a pipelined call's later groups are launched with 256 lanes (512 for
    the schedule, 1024 for k_binscan); read the allocations off the shipped code object and hold them to the rule."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    alloc = kr.allocated_vgprs(pkg.lib_path())
    acc = [v for k, v in alloc.items() if "k_accumulate<msmk::G1C>" in k]
    assert acc and acc[0] <= 216, acc                          # the budget the rule below is derived from: 512 - 2 * 216 = 80
    lanes = {"k_coarse<false": 256, "k_coarse<true": 256, "k_coarse_staged_co<": 256, "k_coarseA<": 256, "k_colscan": 256, "k_binscan": 1024, "k_seg_count": 256,
             "k_fine_count": 256, "k_fine_scan": 256, "k_fine_scatter": 256, "k_mid_count": 256, "k_mid_scan": 512, "k_mid_scatter": 256,
             "k_sched1<512": 512, "k_sched2<512": 512, "k_sched3<512": 512}
    seen = set()
    for name, regs in alloc.items():
        for key, nt in lanes.items():
            if key in name:
                seen.add(key)
                assert (nt // 256) * regs <= 80, (name, nt, regs)
    assert seen == set(lanes), set(lanes) - seen

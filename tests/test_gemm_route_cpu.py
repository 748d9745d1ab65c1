"""The GEMM kernel choice without a GPU: csrc/gemm.hip decides in one function (gemm_route) which kernel a call runs and what follows it,
and include/oasr_testing.h exports that function on plain integers (oasr_gemm_route_debug).  Nothing is launched here.

 1. the hand-written eligibility rule the GPU suite generates its cases from (tests/gemm_exact.py: ``takes``) agrees with the route on a grid
    around every rule's edge;
 2. the automatic route on the medium training step's own launch configurations (symbols as a B = 128 span step recorded them on the MI355X
    with oasr_profile_gemm_records before the route existed) and at each rule's edge;
 3. the route reads its arguments, not the process-wide hooks.
"""
import ctypes
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_exact as gx  # noqa: E402

LAYOUTS = {"NT": (False, False), "NN": (False, True), "TN": (True, False), "TT": (True, True)}
OUT, PRE, F32 = 1, 2, 4                 # `outputs` bits of oasr_gemm_route_debug
BIAS, RESID, U, POS = 1, 2, 4, 8        # `sides` bits
POST_NONE, POST_FROM_OUT, POST_FROM_SCRATCH = 0, 1, 2


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    from olmoasr_amd import _native
    if not os.path.isfile(_native.LIB_PATH):
        g.build()
    return _native


def route(native, M, N, K, layout="NT", *, outputs=OUT, sides=0, a_view=0, b_view=0, split_k=1, atomic=0, atomic_on_pp=0, ldc=None, ldr=None, ldu=None,
          misalign=0, colsum=0, scratch=0, forced=0, schedule=-1, geom_env=0):
    """(kernel symbol, post-step) of one call.  Leading dimensions default to the row length rounded up to 8 plus a pad, as gx.embed lays
    matrices out."""
    ta, tb = LAYOUTS[layout]
    ld = (N + 7) // 8 * 8 + 72
    buf, post = ctypes.create_string_buffer(256), ctypes.c_int(-1)
    rc = native.lib().oasr_gemm_route_debug(M, N, K, int(ta), int(tb), a_view, b_view, split_k, atomic, atomic_on_pp, outputs, sides,
                                            ld if ldc is None else ldc, ld if ldr is None else ldr, ld if ldu is None else ldu, misalign, colsum,
                                            scratch, forced, schedule, geom_env, buf, len(buf), ctypes.byref(post))
    native.check(rc, "oasr_gemm_route_debug")
    return buf.value.decode(), post.value


# ======================================================================================================================================
# 1. takes() against the route
# ======================================================================================================================================
GRID_M, GRID_N, GRID_K = (7, 8, 32, 33, 64, 65, 256), (4, 8, 12, 256, 264), (8, 56, 64, 72, 128)


@pytest.mark.parametrize("path", list(gx.PATHS))
def test_takes_agrees_with_the_forced_route_on_the_edge_grid(native, path):
    """For every point, takes(path, ...) is true exactly when the route, forced as PATHS says, lands in the path's kernel family.  The
    persistent paths carry one more condition in takes -- more 256 x 256 tiles than compute units, unsplit -- which is a property of the
    launch (csrc/gemm_pp.hip), not of the route: it is and-ed to the route's answer here."""
    mode, variant, fam = gx.PATHS[path]
    schedule = -1 if variant < 0 or (variant & 15) == 8 else variant & 15
    wrong = []
    for (lay, (ta, tb)), M, N, K, atomic_only, f32 in itertools.product(LAYOUTS.items(), GRID_M, GRID_N, GRID_K, (False, True), (False, True)):
        outputs, atomic = (F32, 1) if atomic_only else ((OUT | F32, 0) if f32 else (OUT, 0))  # fp32 stores come beside a bf16 `out` in the GPU suite
        symbol, _ = route(native, M, N, K, lay, outputs=outputs, atomic=atomic, forced=mode, schedule=schedule)
        lands = gx.family_of(symbol) == fam
        if path.startswith("pp_persistent"):
            lands = lands and not atomic_only and ((M + 255) // 256) * ((N + 255) // 256) > 256
        if gx.takes(path, M, N, K, ta, tb, atomic_only=atomic_only, f32=f32) != lands:
            wrong.append((lay, M, N, K, atomic_only, f32, symbol))
    assert not wrong, f"{path}: takes() and the route disagree at {len(wrong)} points, first {wrong[:5]}"


# ======================================================================================================================================
# 2. the automatic route
# ======================================================================================================================================
PP, FAST = "oasr_gemm_pp_kernel<%s>", "oasr_gemm_fast_kernel<%s>"
WGRAD_128 = FAST % "true, true, 128, 2, 1, false, false"
# One medium B = 128 span step (807 launches, 42 distinct configurations), as recorded:
# (symbol, M, N, K, layout, epilogue flag word, split_k, atomic, atomic_on_pp, colsum with scratch)
STEP = [
    ("gemm_kernel<false, false>", 128, 1024, 256, "NT", 113, 1, 0, 0, 0),
    ("gemm_kernel<false, false>", 128, 1024, 3072, "NT", 369, 1, 0, 0, 0),
    ("gemm_kernel<true, true>", 1, 1024, 18944, "TT", 0, 16, 1, 0, 0),
    (WGRAD_128, 1024, 1024, 128, "TT", 512, 1, 1, 0, 0),
    (WGRAD_128, 1024, 1024, 18944, "TT", 0, 16, 1, 0, 0),
    (WGRAD_128, 1024, 256, 384000, "TT", 0, 32, 1, 0, 0),
    (WGRAD_128, 1024, 3072, 192000, "TT", 0, 8, 1, 0, 0),
    (WGRAD_128, 1024, 4096, 18944, "TT", 0, 4, 1, 0, 0),
    (WGRAD_128, 1024, 80, 128, "TT", 512, 1, 1, 0, 0),
    (WGRAD_128, 3072, 1024, 18944, "TT", 0, 8, 1, 0, 0),
    (WGRAD_128, 3072, 1024, 192000, "TT", 0, 8, 1, 0, 0),
    (WGRAD_128, 4096, 1024, 18944, "TT", 0, 4, 1, 0, 0),
    (WGRAD_128, 51864, 1024, 18944, "TT", 0, 1, 1, 0, 0),
    (PP % "false, false, true, false, 7", 18944, 1024, 1024, "NT", 33, 1, 0, 0, 0),
    (PP % "false, false, true, false, 7", 18944, 1024, 1024, "NT", 35, 1, 0, 0, 0),
    (PP % "false, false, true, false, 7", 18944, 1024, 4096, "NT", 35, 1, 0, 0, 0),
    (PP % "false, false, true, false, 7", 18944, 3072, 1024, "NT", 33, 1, 0, 0, 0),
    (PP % "false, false, true, false, 7", 18944, 4096, 1024, "NT", 241, 1, 0, 0, 0),
    (PP % "false, false, true, false, 7", 18944, 51968, 1024, "NT", 32, 1, 0, 0, 0),
    (PP % "false, false, true, false, 7", 192000, 1024, 1024, "NT", 35, 1, 0, 0, 0),
    (PP % "false, false, true, false, 7", 192000, 1024, 3072, "NT", 369, 1, 0, 0, 0),
    (PP % "false, false, true, false, 7", 192000, 1024, 4096, "NT", 35, 1, 0, 0, 0),
    (PP % "false, false, true, false, 7", 192000, 2048, 1024, "NT", 33, 1, 0, 0, 0),
    (PP % "false, false, true, false, 7", 192000, 3072, 1024, "NT", 33, 1, 0, 0, 0),
    (PP % "false, false, true, false, 7", 192000, 4096, 1024, "NT", 241, 1, 0, 0, 0),
    (PP % "false, false, true, false, 7", 384000, 1024, 256, "NT", 113, 1, 0, 0, 0),
    (PP % "false, true, true, false, 7", 18944, 1024, 1024, "NN", 32, 1, 0, 0, 0),
    (PP % "false, true, true, false, 7", 18944, 1024, 3072, "NN", 32, 1, 0, 0, 0),
    (PP % "false, true, true, false, 7", 18944, 1024, 4096, "NN", 32, 1, 0, 0, 0),
    (PP % "false, true, true, false, 7", 18944, 1024, 51968, "NN", 32, 1, 0, 0, 0),
    (PP % "false, true, true, false, 7", 192000, 1024, 1024, "NN", 32, 1, 0, 0, 0),
    (PP % "false, true, true, false, 7", 192000, 1024, 2048, "NN", 32, 1, 0, 0, 0),
    (PP % "false, true, true, false, 7", 192000, 1024, 2048, "NN", 34, 1, 0, 0, 0),
    (PP % "false, true, true, false, 7", 192000, 1024, 3072, "NN", 32, 1, 0, 0, 0),
    (PP % "false, true, true, false, 7", 192000, 1024, 4096, "NN", 32, 1, 0, 0, 0),
    (PP % "false, true, true, false, 7", 192000, 3072, 1024, "NN", 32, 1, 0, 0, 0),
    (PP % "false, true, true, true, 2", 18944, 4096, 1024, "NN", 44, 1, 0, 0, 1),
    (PP % "false, true, true, true, 2", 192000, 4096, 1024, "NN", 44, 1, 0, 0, 1),
    (PP % "true, true, false, false, 7", 1024, 1024, 192000, "TT", 0, 16, 1, 1, 0),
    (PP % "true, true, false, false, 7", 1024, 4096, 192000, "TT", 0, 4, 1, 1, 0),
    (PP % "true, true, false, false, 7", 2048, 1024, 192000, "TT", 0, 8, 1, 1, 0),
    (PP % "true, true, false, false, 7", 4096, 1024, 192000, "TT", 0, 8, 1, 1, 0),
]


@pytest.mark.parametrize("case", STEP, ids=[f"{c[0].split('<')[0]}-{c[4]}-{c[1]}x{c[2]}x{c[3]}-f{c[5]}" for c in STEP])
def test_automatic_route_of_the_medium_step(native, case):
    """No path forced: the route names the kernel the step launched.  The facts come from the record: the epilogue flag word says which
    outputs and side inputs the call had (an atomic call has the fp32 output alone), the engine passes colsum always with its scratch rows, and
    the step's matrices are dense and 16-byte aligned (ld = row length).  The two conv-stem launches on the general kernel are window views."""
    symbol, M, N, K, lay, flags, split_k, atomic, on_pp, scratch = case
    outputs = F32 if atomic else ((OUT if flags & 32 else 0) | (PRE if flags & 16 else 0))
    sides = (BIAS if flags & 1 else 0) | (RESID if flags & 2 else 0) | (U if flags & 4 else 0) | (POS if flags & 256 else 0)
    view = int(symbol.startswith("gemm_kernel<false") and M == 128)  # conv1 / conv2 edge rows
    got = route(native, M, N, K, lay, outputs=outputs, sides=sides, a_view=view, split_k=split_k, atomic=atomic, atomic_on_pp=on_pp, ldc=N, ldr=N,
                ldu=N, colsum=scratch, scratch=scratch)
    assert got == (symbol, POST_FROM_SCRATCH if scratch else POST_NONE)


NT128 = FAST % "false, false, 128, 2, 1, true, false"
# (what the case is about, arguments of route(), expected symbol, expected post-step); the expectations follow launch_gemm's rules as written
# before the route existed: skinny for M <= 64 plain NT calls with K % 64 == 0; ping-pong for bf16 outputs with more than 128 tiles of 256 x 256
# and K >= 2 x 64; atomic outputs on 256 x 128 unless atomic_on_pp and M, N % 256 == 0; fused column sums for the NN layout only.
EDGES = [
    ("skinny M = 32", dict(M=32, N=256, K=128), "gemm_skinny_kernel<1>", POST_NONE),
    ("skinny M = 33", dict(M=33, N=256, K=128), "gemm_skinny_kernel<2>", POST_NONE),
    ("skinny M = 64", dict(M=64, N=256, K=128), "gemm_skinny_kernel<2>", POST_NONE),
    ("skinny M = 65", dict(M=65, N=256, K=128), NT128, POST_NONE),
    ("skinny needs K % 64 == 0", dict(M=64, N=256, K=72), "gemm_kernel<false, false>", POST_NONE),
    ("skinny is NT only", dict(M=64, N=256, K=128, layout="NN"), FAST % "false, true, 128, 2, 1, true, false", POST_NONE),
    ("128 tiles", dict(M=256 * 128, N=256, K=128), NT128, POST_NONE),
    ("129 tiles", dict(M=256 * 128 + 8, N=256, K=128), PP % "false, false, true, false, 7", POST_NONE),
    ("129 tiles, K = 64 < 2 BK", dict(M=256 * 128 + 8, N=256, K=64), NT128, POST_NONE),
    ("129 tiles, K = 128 = 2 BK", dict(M=256 * 129, N=256, K=128), PP % "false, false, true, false, 7", POST_NONE),
    ("atomic_on_pp, M % 256 == 0", dict(M=1024, N=1024, K=4096, layout="TT", outputs=F32, atomic=1, split_k=8, atomic_on_pp=1),
     PP % "true, true, false, false, 7", POST_NONE),
    ("atomic_on_pp, M % 256 != 0", dict(M=1032, N=1024, K=4096, layout="TT", outputs=F32, atomic=1, split_k=8, atomic_on_pp=1), WGRAD_128, POST_NONE),
    ("atomic_on_pp, N % 256 != 0", dict(M=1024, N=1032, K=4096, layout="TT", outputs=F32, atomic=1, split_k=8, atomic_on_pp=1), WGRAD_128, POST_NONE),
    ("atomic without atomic_on_pp", dict(M=1024, N=1024, K=4096, layout="TT", outputs=F32, atomic=1, split_k=8), WGRAD_128, POST_NONE),
    ("atomic: many tiles do not make it ping-pong", dict(M=256 * 129, N=256, K=128, layout="TT", outputs=F32, atomic=1), WGRAD_128, POST_NONE),
    ("colsum NN small, scratch", dict(M=640, N=384, K=1024, layout="NN", colsum=1, scratch=1), FAST % "false, true, 128, 2, 1, true, true", POST_FROM_SCRATCH),
    ("colsum NN small, atomics", dict(M=640, N=384, K=1024, layout="NN", colsum=1), FAST % "false, true, 128, 2, 1, true, true", POST_NONE),
    ("colsum NN large, scratch", dict(M=192000, N=4096, K=1024, layout="NN", colsum=1, scratch=1), PP % "false, true, true, true, 2", POST_FROM_SCRATCH),
    ("colsum NN large, atomics", dict(M=192000, N=4096, K=1024, layout="NN", colsum=1), PP % "false, true, true, true, 2", POST_NONE),
    ("colsum NT small", dict(M=640, N=384, K=1024, colsum=1, scratch=1), NT128, POST_FROM_OUT),
    ("colsum NT large", dict(M=192000, N=4096, K=1024, colsum=1, scratch=1), PP % "false, false, true, false, 7", POST_FROM_OUT),
    ("colsum TN small", dict(M=640, N=384, K=1024, layout="TN", colsum=1), FAST % "true, false, 128, 2, 1, true, false", POST_FROM_OUT),
    ("colsum TT large", dict(M=192000, N=4096, K=1024, layout="TT", colsum=1, scratch=1), PP % "true, true, true, false, 7", POST_FROM_OUT),
    ("colsum on the general kernel (K % 64 != 0)", dict(M=640, N=384, K=200, layout="NN", colsum=1, scratch=1), "gemm_kernel<false, true>", POST_FROM_OUT),
    ("colsum NN forced onto 256 x 256 two-stage: not fused", dict(M=640, N=384, K=1024, layout="NN", colsum=1, scratch=1, forced=3),
     FAST % "false, true, 256, 4, 2, true, false", POST_FROM_OUT),
    ("fp32 store beside out", dict(M=640, N=384, K=1024, outputs=OUT | F32), "gemm_kernel<false, false>", POST_NONE),
    ("out not 16-byte aligned", dict(M=640, N=384, K=1024, misalign=8), "gemm_kernel<false, false>", POST_NONE),
    ("ldc % 8 != 0", dict(M=640, N=384, K=1024, ldc=388), "gemm_kernel<false, false>", POST_NONE),
    ("resid with ldr % 8 != 0", dict(M=640, N=384, K=1024, sides=RESID, ldr=388), "gemm_kernel<false, false>", POST_NONE),
    ("pos with a side input", dict(M=640, N=384, K=1024, sides=POS | RESID), "gemm_kernel<false, false>", POST_NONE),
    ("pos alone", dict(M=640, N=384, K=1024, sides=POS | BIAS), NT128, POST_NONE),
    ("window view of B", dict(M=640, N=384, K=1024, b_view=1), "gemm_kernel<false, false>", POST_NONE),
    ("schedule override 2", dict(M=192000, N=1024, K=1024, schedule=2), PP % "false, false, true, false, 2", POST_NONE),
    ("schedule override 7 on the fused dgrad", dict(M=192000, N=4096, K=1024, layout="NN", colsum=1, scratch=1, schedule=7),
     PP % "false, true, true, true, 7", POST_FROM_SCRATCH),
    ("OASR_GEMM_GEOM=3 on a small problem", dict(M=640, N=384, K=1024, geom_env=3), PP % "false, false, true, false, 7", POST_NONE),
    ("OASR_GEMM_GEOM=1 on a large problem", dict(M=192000, N=1024, K=1024, geom_env=1), NT128, POST_NONE),
    ("a forced path outranks OASR_GEMM_GEOM", dict(M=640, N=384, K=1024, geom_env=3, forced=2), NT128, POST_NONE),
]


@pytest.mark.parametrize("what,args,symbol,post", EDGES, ids=[e[0].replace(" ", "_") for e in EDGES])
def test_automatic_route_at_each_rules_edge(native, what, args, symbol, post):
    args = dict(args)
    M, N, K = args.pop("M"), args.pop("N"), args.pop("K")
    assert route(native, M, N, K, args.pop("layout", "NT"), **args) == (symbol, post), what


# ======================================================================================================================================
# 3. the route reads its arguments only
# ======================================================================================================================================
def test_route_does_not_read_the_process_wide_hooks(native, monkeypatch):
    lib = native.lib()
    monkeypatch.setenv("OASR_TESTING_HOOKS", "1")
    calls = [dict(M=192000, N=1024, K=1024), dict(M=64, N=256, K=128), dict(M=640, N=384, K=1024, layout="NN", colsum=1, scratch=1)]

    def answers():
        out = []
        for c in calls:
            c = dict(c)
            out.append(route(native, c.pop("M"), c.pop("N"), c.pop("K"), c.pop("layout", "NT"), **c))
        return out
    before = answers()
    assert [gx.family_of(s) for s, _ in before] == ["pp", "skinny", "fast128"]
    try:
        assert lib.oasr_gemm_force_general(1) == 0  # every launch now takes the general kernel ...
        assert lib.oasr_gemm_set_variant(2) == 0
        assert answers() == before                  # ... and the route, asked with forced_path = 0, answers as before
    finally:
        assert lib.oasr_gemm_force_general(0) == 0
        assert lib.oasr_gemm_set_variant(-1) == 0

"""tests/dispatch_rules.py on the CPU: the restated rules against the figures the sources and the GPU-checked points of
tests/test_gpu_dispatch_edges.py state, and the collection-time assertions of the dispatch-edge test files (importing them runs
them: every parametrized point must sit on the side of its rule that its comment claims)."""
import importlib

import dispatch_rules as R


def test_ms_fits_reproduces_the_pool_counts_the_sweep_tests_sit_on():
    # MODE 0 (test_gpu_dispatch_edges.py, section B) and MODE 2 (section C): last matrix-core pool counts, run there on both sides
    assert [R.last_ms_count(cu, 0) for cu in (2, 3, 4, 6, 8, 12, 16, 17, 32, 33, 34)] == [1176, 1120, 1120, 1056, 960, 864, 728, 336, 112, 240, 240]
    assert [R.last_ms_count(1 + k, 2) for k in (1, 3, 15)] == [1120, 1056, 672]
    assert [R.ms_pick_u((n + 7) // 8) for n in (285, 301, 513, 777, 1000, 1176)] == [6, 8, 5, 7, 5, 7]
    assert not R.ms_fits(32, 2, 1) and R.ms_fits(33, 2, 1) and not R.ms_fits(200, 49, 1)
    assert [R.round_cols(c) for c in (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 34, 35)] == [2, 2, 3, 4, 6, 8, 12, 16, 24, 34, 34, -1]


def test_coefficient_pass_routes_cover_every_kernel_and_width():
    seen = {R.beta_route(n, c, colmajor=cm, ss=ss, env=env)
            for n in range(2, 1300) for c in (1, 2, 3, 4, 6, 8, 12, 16, 20, 30, 34) for cm in (False, True) for ss in (False,)
            for env in ((), ("OLD", "VALU"), ("OLD", "VALU", "SCALAR"))}
    assert {("beta_scalar", c) for c in R.COL_SIZES} <= seen and {("beta_lds", c) for c in (6, 8, 12, 16, 24)} <= seen
    assert ("beta_mfma", 16) in seen and {("matrix-core", c) for c in R.COL_SIZES} <= seen
    assert not any(r == "beta_lds" and c in (2, 3, 4, 34) for r, c in seen)
    # g'g (ss_out_dev) is written by the matrix-core mode and the scalar kernel only
    assert {R.beta_route(n, c, colmajor=False, ss=True, env=env)[0] for n in range(3, 1300) for c in (2, 6, 10)
            for env in ((), ("OLD",))} == {"matrix-core", "beta_scalar"}


def test_batched_passes_and_geometry_figures_of_the_sources():
    passes, short = R.batched_passes(10, 1, 10)                    # pg_gp.hip:866: config 4, 101 columns, 7 passes instead of 11
    assert sum(passes) == 101 and len(passes) == 7 and short and passes[0] == 10
    assert [R.path_lp(L) for L in range(2, 17)] == [2, 4, 4, 6, 6, 8, 8, 10, 10, 12, 12, 14, 14, 16, 16]
    assert R.predict_geometry(500, 10, 11) == dict(LPr=12, chunk=41, threads=512, groups=1, grid_y=1, lds=8 * 41 * 10 * 14 + 2640,
                                                   variant=(12, False, True))
    assert [R.mass_nb(p) for p in (1, 65536, 67583, 67584, 2097152, 2099199, 10 ** 7)] == [32, 32, 32, 33, 1024, 1024, 1024]
    assert R.fst_chunk(1500) == (64, 24, 28) and R.fst_slab(200, 10) == 10 and R.fst_slab(200, 10 ** 6) == 3355


def test_kinship_layouts_of_the_sources():
    assert R.kin_layout(17 * 16)["Tb"] == 6 and R.kin_layout(14 * 16)["Tb"] == 8       # pg_kinship.hip:706-709: 6 + 6 + 5, 8 + 6
    assert [R.kin_layout(n)["nb"] for n in (208, 209, 256, 257, 384, 385, 640)] == [1, 2, 2, 3, 3, 4, 5]
    assert R.kin_layout(64)["w8"] and not R.kin_layout(65)["w8"]


def test_every_dispatch_edge_point_sits_where_its_comment_says():
    for name in ("test_gpu_dispatch_edges_gp", "test_gpu_dispatch_edges_popgen", "test_gpu_kinship_path"):
        importlib.import_module(name)                               # the module-level assertions run on import

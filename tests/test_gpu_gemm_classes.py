"""Every kernel class and descriptor flag of the grouped GEMM (dm_gemm.hip) against the long-double reference of
tests/gemm_cases.py, element by element with its derived bound, through dm_zgemm_grouped_ex.  The references are
computed once per process (gemm_cases.cached)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gemm_cases as gc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gc.LD_OK, reason="np.longdouble has no 64-bit mantissa here")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from driftscan_amd._lib import Context

    c = Context(0, workspace_bytes=1 << 28)
    yield c
    c.close()


@pytest.mark.parametrize("group", [g for g in gc.GROUPS if g != "chunk"])
def test_each_case_in_a_launch_of_its_own(ctx, group):
    """One call, one launch per case: the deep and the wide decisions are taken per launch, so a K >= 512 case runs on
    the deep kernel here and an N >= 160 real-B case on the 64 x 128 tiles.  The deep cases leave 2, 3 and 4 steps to
    the rotating loop's remainder (K = 512, 516, 520) and add the masked tail (513, 518, 523), on interior and on
    ragged tiles.  Short K (8 .. 24, nfull 2 .. 6) would reach that loop only under a forced DM_GEMM4_DEEP, an
    experiment switch read once per process that is not tested."""
    names = [c["name"] for c in gc.group_cases(group) if c["solo"] and c["groups"][0] == group]
    fails = gc.run_and_check(ctx, names, solo=True)
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("group", gc.GROUPS)
def test_class_launch(ctx, group):
    """All cases of a group in ONE launch: 'complex' mixes K < 512 with the deep cases (none runs deep), 'deep' holds
    only K >= 512, 'real_narrow' / 'real_wide' put wide problems on 64-wide tiles and narrow ones on 128-wide tiles,
    'mixed' holds all four classes with empty problems in between and K rising (the longest-first sort reorders the
    tiles), 'chunk' has more tiles per class than one round of XCD chunks."""
    fails = gc.run_and_check(ctx, [c["name"] for c in gc.group_cases(group)], solo=False)
    assert not fails, "\n".join(fails[:20])


def test_chain_of_dependent_launches(ctx):
    """Three products in one call, each reading the C of the one before as its A (plans built first, one upload, run
    in launch order).  Each link is checked against the long-double reference of what it actually read, and the three
    results are bit-identical to the same products issued as three calls."""
    ds = [gc.materialise(c) for c in gc.CHAIN]

    def issue(one_call):
        tens = [gc.upload(ctx, d) for d in ds]
        probs = []
        for i, d in enumerate(ds):
            (p,) = gc.problems(d, launch=i)
            p.update(A=tens[i][0], B=tens[i][1], C=tens[i][2], kscale=None)
            if i > 0:   # A = the view of the previous C
                p.update(A=tens[i - 1][2], a_off=ds[i - 1].c_off, rsA=ds[i - 1].ldc, csA=ds[i - 1].csc)
            probs.append(p)
        if one_call:
            ctx.zgemm_grouped_ex(probs)
        else:
            for p in probs:
                ctx.zgemm_grouped_ex([p])
        ctx.sync()
        return [t[2].cpu().numpy() for t in tens]

    chained, apart = issue(True), issue(False)
    for a, b in zip(chained, apart):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    fails = []
    for i, c in enumerate(gc.CHAIN):
        d = gc.materialise(c, A_values=chained[i - 1][ds[i - 1].iC] if i > 0 else None)
        assert np.array_equal(d.C_buf.view(np.uint64), ds[i].C_buf.view(np.uint64))
        assert np.array_equal(d.B_buf[d.iB], ds[i].B_buf[d.iB])
        fails += gc.check(d, gc.reference(d), chained[i])
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("label,prob", gc.refused_problems(), ids=[x[0] for x in gc.refused_problems()])
def test_refused_combinations_touch_nothing(ctx, label, prob):
    """Each flag combination that a kernel class would silently ignore is refused, alone and behind a good launch of
    the same call, and no output buffer changes."""
    from driftscan_amd import _lib

    torch = ctx.torch
    real = lambda f, b: torch.float64 if f & b else torch.complex128   # noqa: E731
    f = prob["flags"]

    def tensors(flags):
        A = torch.ones(256, dtype=real(flags, _lib.ZGEMM_ALL_REAL), device="cuda")
        B = torch.ones(256, dtype=real(flags, _lib.ZGEMM_ALL_REAL | _lib.ZGEMM_B_REAL), device="cuda")
        C = torch.full((256,), 7.0, dtype=real(flags, _lib.ZGEMM_ALL_REAL), device="cuda")
        return A, B, C

    A, B, C = tensors(f)
    ks = torch.ones(64, dtype=torch.float64, device="cuda") if prob.get("has_kscale") else None
    bad = dict(prob, A=A, B=B, C=C, kscale=ks, launch=1)
    A0, B0, C0 = tensors(0)
    good = dict(M=8, N=8, K=4, rsA=4, csA=1, rsB=8, csB=1, ldc=8, A=A0, B=B0, C=C0, launch=0)
    for probs in ([bad], [good, bad]):
        with pytest.raises(_lib.DriftMIError):
            ctx.zgemm_grouped_ex(probs)
        ctx.sync()
        assert bool((C == 7.0).all()) and bool((C0 == 7.0).all())
    ctx.zgemm_grouped_ex([good])   # the good launch alone runs: 4 * (1 + 0i)(1 + 0i)
    ctx.sync()
    assert bool((C0[:64] == 4.0).all()) and bool((C0[64:] == 7.0).all())


def test_lds_fallback_in_a_child_process(ctx, tmp_path):
    """DM_GEMM4=0 (read once per process, hence the child): the complex, real-B and gathered cases and the chunk-remap
    launch on the LDS-staged kernels, against the same table and references."""
    cache = str(tmp_path / "gemm_cases.pkl")
    gc.save_cache(cache, gc.child_names())
    script = ("import sys\n"
              "sys.path[:0] = [%r, %r]\n"
              "import gemm_cases\n"
              "sys.exit(gemm_cases.child_main(%r))\n") % (ROOT, os.path.join(ROOT, "tests"), cache)
    res = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, DM_GEMM4="0"), capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-3000:], res.stderr[-2000:])

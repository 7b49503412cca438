"""The bounds of tests/test_gpu_batchnorm.py, checked without a GPU: a numpy float32 restatement of bn_stats_part_kernel /
bn_stats_final_kernel (csrc/batchnorm.hip: sums shifted by the chunk's first live row, Chan's merge in four interleaved partials)
is held against the float64 reference of the SAME cases with the SAME bound functions and must stay within HALF of every bound; a
plain f32 E[x^2] - E[x]^2 over the same rows must EXCEED the bounds on the cancellation profiles b (mean 1e3, std 1e-2) and f
(mean -7, std 1e-3).  So the inputs discriminate and the bounds are not loose.  (The restatement rounds every operation; the device
code contracts a * b + c into one rounding, which only removes roundings.)"""
import numpy as np
import pytest

import test_gpu_batchnorm as B

f32 = np.float32
ROW_CASES = [(nr, p) for nr in B.ROW_EDGES for p in (None, "cyc7", "first_dead", "dead_chunk") if p != "dead_chunk" or nr >= 255]


def chan_merge(n, mean, M2, nb, mb, m2b):
    """chan_merge of csrc/batchnorm.hip on [C] float32 vectors; columns with nb == 0 are left alone."""
    with np.errstate(divide="ignore", invalid="ignore"):
        nt = n + nb
        dlt = mb - mean
        mean2 = mean + dlt * (nb / nt)
        M22 = M2 + (m2b + dlt * dlt * (n * nb / nt))
    skip = nb == 0
    return np.where(skip, n, nt), np.where(skip, mean, mean2), np.where(skip, M2, M22)


def f32_stats(c, rep=1):
    """mean, rstd, run_mean, run_var as the kernels compute them, every operation rounded to float32."""
    NR, C, rpc, nch = c.NR, c.C, c.rpc, c.nch
    pad = nch * rpc - NR
    x = np.concatenate([c.x, np.zeros((pad, C), f32)]).reshape(nch, rpc, C)
    live = np.concatenate([c.live, np.zeros(pad, bool)]).reshape(nch, rpc)
    K, s1, s2 = (np.zeros((nch, C), f32) for _ in range(3))
    cnt = np.zeros(nch, np.int64)
    for i in range(rpc):
        ok = live[:, i]
        v = np.where(ok[:, None], x[:, i], f32(0))                     # (dead rows hold NaN: never read)
        K = np.where((ok & (cnt == 0))[:, None], v, K)
        dlt = np.where(ok[:, None], v - K, f32(0))
        s1 = s1 + dlt
        s2 = s2 + dlt * dlt
        cnt += ok
    assert s1.dtype == s2.dtype == f32
    inv = np.where(cnt > 0, f32(1) / np.maximum(cnt, 1).astype(f32), f32(0)).astype(f32)[:, None]
    pn = np.broadcast_to(cnt.astype(f32)[:, None], (nch, C))
    pm = K + s1 * inv
    pq = s2 - s1 * s1 * inv
    waves = []
    for w in range(4):
        n, mean, M2 = (np.zeros(C, f32) for _ in range(3))
        for b in range(w, nch, 4):
            n, mean, M2 = chan_merge(n, mean, M2, pn[b], pm[b], pq[b])
        waves.append((n, mean, M2))
    n, mean, M2 = waves[0]
    for w in range(1, 4):
        n, mean, M2 = chan_merge(n, mean, M2, *waves[w])
    assert mean.dtype == M2.dtype == f32
    with np.errstate(divide="ignore", invalid="ignore"):
        var = np.where(n > 0, M2 / n, f32(0)).astype(f32)
        rstd = f32(1) / np.sqrt(var + f32(B.EPS))
        mom, r = f32(B.MOM), f32(rep)
        unb = np.where(n * r > 1, M2 * r / (n * r - f32(1)), var).astype(f32)
    return mean, rstd.astype(f32), (f32(1) - mom) * c.rm0 + mom * mean, (f32(1) - mom) * c.rv0 + mom * unb


def naive_stats(c):
    """E[x^2] - E[x]^2 in float32 (numpy's pairwise sums: kinder than a running sum)."""
    xl = c.x[c.rows]
    n = f32(c.n)
    mean = xl.sum(0, dtype=f32) / n
    var = (xl * xl).sum(0, dtype=f32) / n - mean * mean
    with np.errstate(invalid="ignore", divide="ignore"):
        return mean, f32(1) / np.sqrt(np.maximum(var, f32(0)) + f32(B.EPS))


WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n[batchnorm bounds] float32 restatement, worst error / bound: %s" % ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


@pytest.mark.parametrize("NR,pattern", ROW_CASES, ids=["%d-%s" % c for c in ROW_CASES])
def test_float32_restatement_stays_within_half_of_every_bound(NR, pattern):
    for bf16 in (False, True):
        c = B.case(NR, 8, pattern, bf16)
        for rep in (1, 5):
            mean, rstd, rm, rv = f32_stats(c, rep)
            cc = c.constant
            assert (mean[cc].astype(np.float64) == c.mean[cc]).all() and np.unique(rstd[cc].view(np.int32)).size <= 1
            got = {"mean": (mean, c.mean, B.mean_tol(c)), "rstd": (rstd, c.rstd, B.rstd_rtol(c) * c.rstd),
                   "run_mean": (rm, (1 - B.MOM) * c.rm0.astype(np.float64) + B.MOM * c.mean, B.run_mean_tol(c)),
                   "run_var": (rv, (1 - B.MOM) * c.rv0.astype(np.float64) + B.MOM * c.var_unbiased(rep), B.run_var_tol(c, rep))}
            for what, (g_, ref, tol) in got.items():
                r = B._ratio(np.abs(g_.astype(np.float64) - ref), tol)
                WORST[what] = max(WORST.get(what, 0.0), r)
                assert r <= 0.5, (what, NR, pattern, bf16, rep, r)


def test_the_bounds_admit_what_a_correct_float32_evaluation_does():
    """Profile b at 32769 rows: the mean bound is a fraction of one standard deviation and the rstd bound a fraction of a percent,
    well above what float32 needs there and far below the naive formulation's error; benign columns are held to a few 1e-6."""
    c = B.case(32769, 8, None)
    b, a, h = 1, 0, 7
    assert (c.nch, c.rpc) == (257, 128)
    assert 1.4e-2 * 2 <= B.mean_tol(c)[b] / np.sqrt(c.var[b]) <= 0.25
    assert 1.2e-4 * 2 <= B.rstd_rtol(c)[b] <= 5e-2
    assert 2e-6 <= B.rstd_rtol(c)[a] <= 1e-5 and B.rstd_rtol(c)[h] <= 1e-4


@pytest.mark.parametrize("NR", [255, 32768, 32769])
def test_naive_float32_variance_exceeds_the_bounds_on_the_cancellation_profiles(NR):
    c = B.case(NR, 8, "cyc7")
    assert c.n > 100
    mean, rstd = naive_stats(c)
    err = np.abs(rstd.astype(np.float64) - c.rstd) / c.rstd
    tol = B.rstd_rtol(c)
    for col, name in ((1, "b"), (5, "f")):
        assert B.PROFILES[col] == name
        assert err[col] > 1e-2 and err[col] > 4 * tol[col], (name, err[col], tol[col])
    # ... while the chunked evaluation of the very same rows is inside
    _, rstd_c, _, _ = f32_stats(c)
    assert (np.abs(rstd_c.astype(np.float64) - c.rstd) / c.rstd <= 0.5 * tol).all()

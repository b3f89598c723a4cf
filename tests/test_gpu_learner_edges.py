"""The learner kernels per parameter block at the edges of their 32-sample tile: dm_vf_fit_epoch, dm_ppo_lossgrad and dm_disc_lossgrad through
the C ABI against float64 numpy references of the same float32-rounded inputs (tests/learner_cases.py builds every case and its reference on
the CPU; tests/test_learner_blocks.py checks them there), every gradient compared block by block (tests/learner_blocks.py), and the forward
kernels' outputs past `n`.

  a. value fit    two minibatches of bs in {1, 31, 32, 33, 96, 160, 2049} rows (1, 1, 1, 2, 3, 5, 65 blocks: quarter_sum's single block, its
                  empty last quarter, its first full group of sixteen) from a non-zero filter and non-zero Adam moments, in both forms of the
                  filter; Adam's m (linear in the gradient) and v (quadratic) per block after EACH minibatch, theta against the Adam rule
                  replayed in float64, the filter's state;
  b. PPO          n in {1, 31, 32, 33, 65}, rows 0 .. n - 1 and rows gathered with replacement (a row three times in one tile, a row in two
                  tiles), entcoeff 0.01; three constructed minibatches of 33 rows: all clipped, all advantages zero, clip = 0;
  c. discriminator (ng, ne) in {(1, 1), (32, 32), (31, 33), (33, 31), (1, 65), (65, 1)} x entcoeff in {1e-3, 1}; saturated logits at (33, 31);
  d. rows past n  dm_policy_act (n in {1, 15, 16, 17, 33}), dm_pg_losses' old_mean and dm_disc_reward's reward (n in {1, 31, 33}): 32 more rows
                  of every output, prefilled, must keep their bits.

The bar is the project's 1e-4 for these kernels (tests/test_gpu_ppo.py, tests/test_gpu_gail.py), here of each BLOCK's largest reference entry.
Bars set from a float32 envelope instead (4 x the error of the same numpy formulas evaluated in float32 against float64, on the same case):

    case | block | float32 envelope | bar
    -----+-------+------------------+----
    none: on an MI355X the worst block of any case is 5.4e-7 (value fit, m and v), 6.4e-6 (PPO), 7.8e-7 (discriminator) and 9.4e-7 (policy
    gradient) of the block's largest entry, so every block keeps the bar of 1e-4.

Every test prints its figures (the worst block and its error as a fraction of the block's largest entry) before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import _abi as A
from tests import bc_numpy as BN
from tests import gail_numpy as GN
from tests import learner_blocks as LB
from tests import learner_cases as LC

DEV = "cuda:0"
PAD = 32                                                               # rows past n of an output: a whole tile more
SENTINEL = -12345.678


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _report(what, got, ref, blocks):
    e = LB.block_errors(got, ref, blocks)
    k = max(e, key=e.get)
    print("%s: worst block %s %.3g" % (what, k, e[k]))


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


# ---- a. the value fit -------------------------------------------------------------------------------------------------------------------
def _vf_fit(c, nb, epoch_filter):
    """dm_vf_fit_epoch on the first nb minibatches of the case, from its start state -> dict of numpy arrays"""
    L = A.load()
    th, m, v = (_dev(c[k]).clone() for k in ("theta0", "m0", "v0"))
    s, q, cnt = _dev(c["sum0"]), _dev(c["sumsq0"]), _dev(np.array([c["count0"]]))
    mean, std = (torch.full((56,), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2))
    ob, ret = _dev(c["ob"]), _dev(c["ret"])
    scratch = torch.empty(int(L.dm_vf_scratch_bytes(nb, c["bs"])), dtype=torch.uint8, device=DEV)
    assert th.data_ptr() % 16 == 0
    A.check(L.dm_vf_fit_epoch(_p(ob), _p(ret), nb, c["bs"], _p(th), _p(m), _p(v), (C.c_float * nb)(*c["scales"][:nb]), c["beta1"], c["beta2"], c["eps"],
                              _p(s), _p(q), _p(cnt), _p(mean), _p(std), _p(scratch), _stream(), epoch_filter), L)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in dict(theta=th, m=m, v=v, sum=s, sumsq=q, count=cnt, mean=mean, std=std).items()}


@pytest.mark.gpu
@pytest.mark.parametrize("epoch_filter", [0, 1])
@pytest.mark.parametrize("bs", LC.VF_BS)
def test_value_fit_epoch_matches_float64_per_block(bs, epoch_filter):
    c = LC.vf_case(bs)
    ref = c["ref"]
    one, two = _vf_fit(c, 1, epoch_filter), _vf_fit(c, 2, epoch_filter)
    before = dict(theta=c["theta0"])
    for i, (got, start) in enumerate(((one, before), (two, one))):
        what = "vf bs=%d filter=%d minibatch %d" % (bs, epoch_filter, i)
        for k in ("m", "v"):
            _report(what + " " + k, got[k], ref[i][k], LB.VALUE)
        # the filter this minibatch normalised with (after the epoch: the state the call leaves)
        np.testing.assert_allclose(got["mean"], ref[i]["mean"], rtol=1e-6, atol=0)
        np.testing.assert_allclose(got["std"], ref[i]["std"], rtol=1e-6, atol=0)
        # Adam's moments: m is linear in the gradient, v quadratic — the gradient is judged here, block by block
        LB.assert_blocks(got["m"], ref[i]["m"], LB.VALUE, LB.BAR, what + " m")
        LB.assert_blocks(got["v"], ref[i]["v"], LB.VALUE, LB.BAR, what + " v")
        # theta: the Adam rule replayed in float64 from the moments the kernel holds and the parameters the minibatch started from.  The
        # kernel's step is four correctly rounded float32 operations (a product, a square root, a sum, a quotient), each within 2^-24 of its
        # result: 2^-22 |step| = 2 float32 ulps of the step's length (ulp = 2^-23 |step|; an IEEE float32 evaluation of the same formula on
        # the CPU reaches 2.9 spacings at the step's own binade, so the spacing there is too small a unit).  Storing theta in float32
        # rounds once more, by half a spacing of theta.  That store term dominates: with theta near 0.1 and steps near 1e-4 it is ~3.7e-9
        # against ~2.4e-11, so in effect theta must be the correctly rounded float32 of (theta - step) — which still sees a step that is
        # wrong by a few 1e-5 of its length; the gradient itself is judged through m and v above.
        step = c["scales"][i] * got["m"].astype(np.float64) / (np.sqrt(got["v"].astype(np.float64)) + c["eps"])
        want = start["theta"].astype(np.float64) - step
        tol = 2.0 * float(np.finfo(np.float32).eps) * np.abs(step) + 0.5 * np.spacing(np.maximum(np.abs(want), np.abs(got["theta"])).astype(np.float32)).astype(np.float64)
        err = np.abs(got["theta"].astype(np.float64) - want)
        print("%s theta: worst %.3g of its tolerance, largest step %.3g" % (what, (err / tol).max(), np.abs(step).max()))
        assert (err <= tol).all(), (what, int((err > tol).sum()), (err / tol).max())
        assert np.abs(step).max() > 1e-5                                # (the step moved the parameters)
    rms = c["rms_after"]
    np.testing.assert_allclose(two["sum"], rms.sum, rtol=1e-12, atol=0)
    np.testing.assert_allclose(two["sumsq"], rms.sumsq, rtol=1e-12, atol=0)
    assert float(two["count"][0]) == rms.count and float(one["count"][0]) == c["count0"] + bs
    # the call with one minibatch is the first minibatch of the call with two: the second really started from moved parameters
    assert not np.array_equal(one["theta"], two["theta"]) and not np.array_equal(one["mean"], two["mean"])


# ---- b. PPO -------------------------------------------------------------------------------------------------------------------------------
NTH = LB.NPOL + LB.NVAL


@pytest.fixture(scope="module")
def ppo():
    S = LC.ppo_data()
    return dict(S=S, D={k: _dev(v) for k, v in S["d"].items()}, th=_dev(LC.f32(S["theta"])), rms=(_dev(LC.f32(S["mean"])), _dev(LC.f32(S["std"]))))


def _ppo_lossgrad(P, D, n, idx, clip, ent=LC.PPO_ENT, grad=True):
    L = A.load()
    scratch = torch.empty(int(L.dm_ppo_scratch_bytes(n if grad else 1)), dtype=torch.uint8, device=DEV)
    out = torch.full((6,), float("nan"), dtype=torch.float64, device=DEV)
    g = torch.full((NTH,), float("nan"), dtype=torch.float32, device=DEV) if grad else None
    idx_d = torch.as_tensor(idx, dtype=torch.int32, device=DEV) if idx is not None else None
    A.check(L.dm_ppo_lossgrad(_p(D["ob"]), _p(D["ac"]), _p(D["atarg"]), _p(D["old_mean"]), _p(D["old_logstd"]), _p(D["ret"]), _p(idx_d), n, _p(P["th"]),
                              _p(P["rms"][0]), _p(P["rms"][1]), clip, ent, _p(g), _p(out), _p(scratch), scratch.numel(), _stream()), L)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (g.cpu().numpy() if grad else None)


def _check_ppo(P, D, d, rows, n, idx, clip, ref, what):
    losses, g = _ppo_lossgrad(P, D, n, idx, clip)
    lref, gref = ref
    _report(what, g, gref, LB.PPO)
    print("%s: losses %s against %s" % (what, losses, lref))
    for k in range(5):
        assert abs(losses[k] - lref[k]) <= 2e-5 * abs(lref[k]) + 1e-9, (what, k, losses[k], lref[k])
    # clipfrac: a row at the clip's edge may count either way in float32 (the existing bar, 2 / n); where the float64 ratios all stay
    # 1e-3 off the edge — a thousand times the float32 error of a ratio of O(1) — the count must be exact
    S = P["S"]
    sub = {k: (v if k == "old_logstd" else v[rows]) for k, v in d.items()}
    ratio = LC.ppo_ratio(S["theta"], S["mean"], S["std"], sub)
    assert abs(losses[5] - lref[5]) <= (2.0 / n if (np.abs(np.abs(ratio - 1.0) - clip) < 1e-3).any() else 1e-12), (what, losses[5], lref[5])
    LB.assert_blocks(g, gref, LB.PPO, LB.BAR, what)
    lonly, _ = _ppo_lossgrad(P, D, n, idx, clip, grad=False)         # the losses alone (no gradient): the same numbers, bit for bit
    assert np.array_equal(lonly, losses), (what, lonly, losses)
    return losses, g


@pytest.mark.gpu
@pytest.mark.parametrize("gathered", [False, True])
@pytest.mark.parametrize("n", LC.PPO_N)
def test_ppo_lossgrad_matches_float64_per_block(ppo, n, gathered):
    c = LC.ppo_case(n, gathered)
    _check_ppo(ppo, ppo["D"], ppo["S"]["d"], c["rows"], n, c["idx"], c["clip"], c["ref"], "ppo n=%d gathered=%d" % (n, gathered))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["clipped", "zero_adv", "clip0"])
def test_ppo_constructed_minibatches(ppo, kind):
    c = LC.ppo_constructed(kind)
    D = {k: _dev(v) for k, v in c["d"].items()}
    losses, g = _check_ppo(ppo, D, c["d"], np.arange(c["n"]), c["n"], None, c["clip"], c["ref"], "ppo " + kind)
    for name, o, k in LB.PPO:
        if name in c["zero"]:
            assert not g[o:o + k].any(), (kind, name, np.flatnonzero(g[o:o + k])[:8])      # exactly 0.0: no row sends a gradient to the mean
    if c["zero"]:
        assert np.array_equal(g[LB.NPOL - 28:LB.NPOL], np.full(28, -np.float32(LC.PPO_ENT)))      # logstd: the entropy penalty alone
    if kind == "clipped":
        assert losses[5] == 1.0
    if kind == "zero_adv":
        assert losses[0] == 0.0


# ---- c. the discriminator -----------------------------------------------------------------------------------------------------------------
def _disc_lossgrad(c):
    L = A.load()
    ng, ne = c["ng"], c["ne"]
    t = {k: _dev(c[k]) for k in ("theta", "mean", "std", "g_ob", "g_ac", "e_ob", "e_ac")}
    scratch = torch.empty(int(L.dm_disc_scratch_bytes(ng, ne)), dtype=torch.uint8, device=DEV)
    out = torch.full((6,), float("nan"), dtype=torch.float64, device=DEV)
    g = torch.full((LB.NDISC,), float("nan"), dtype=torch.float32, device=DEV)
    A.check(L.dm_disc_lossgrad(_p(t["theta"]), _p(t["mean"]), _p(t["std"]), _p(t["g_ob"]), _p(t["g_ac"]), ng, _p(t["e_ob"]), _p(t["e_ac"]), ne,
                               c["entcoeff"], _p(g), _p(out), _p(scratch), scratch.numel(), _stream()), L)
    torch.cuda.synchronize()
    return out.cpu().numpy(), g.cpu().numpy()


def _check_disc_losses(c, losses, what, boundary):
    """the existing bars on the four losses; the accuracies: exact unless a float64 logit lies within `boundary` of 0, then one sample a side"""
    lref = c["ref"][0]
    print("%s: losses %s against %s" % (what, losses, lref))
    assert np.isfinite(losses).all()
    assert np.allclose(losses[:4], lref[:4], rtol=1e-4, atol=1e-6), (what, losses, lref)
    f = LC.f64
    for k, ob, ac, n in ((4, c["g_ob"], c["g_ac"], c["ng"]), (5, c["e_ob"], c["e_ac"], c["ne"])):
        lg = GN.forward(f(c["theta"]), f(c["mean"]), f(c["std"]), f(ob), f(ac))[3]
        assert abs(losses[k] - lref[k]) <= (1.0 / n if (np.abs(lg) < boundary).any() else 0.0) + 1e-12, (what, k, losses[k], lref[k])


@pytest.mark.gpu
@pytest.mark.parametrize("entcoeff", LC.DISC_ENT)
@pytest.mark.parametrize("ng,ne", LC.DISC_SHAPES)
def test_disc_lossgrad_matches_float64_per_block(ng, ne, entcoeff):
    c = LC.disc_case(ng, ne, entcoeff)
    what = "disc ng=%d ne=%d entcoeff=%g" % (ng, ne, entcoeff)
    losses, g = _disc_lossgrad(c)
    losses2, g2 = _disc_lossgrad(c)
    assert np.array_equal(g, g2) and np.array_equal(losses, losses2)   # fixed reduction order
    _report(what, g, c["ref"][1], LB.DISC)
    _check_disc_losses(c, losses, what, 1e-3)                          # (float32 logits of O(1) are within ~1e-5 of the float64 ones)
    LB.assert_blocks(g, c["ref"][1], LB.DISC, LB.BAR, what)


@pytest.mark.gpu
def test_disc_lossgrad_with_saturated_logits():
    c = LC.disc_case(33, 31, 1e-3, logit_scale=14.0)
    losses, g = _disc_lossgrad(c)
    _check_disc_losses(c, losses, "disc saturated", np.inf)            # at most one boundary sample per side
    assert np.isfinite(g).all()
    # the gradient too, block by block: only w3 is scaled up, so d total / d logit saturates at 0, 1 / ng or -1 / ne (float32 keeps
    # those to an ulp) and the hidden layers are those of the moderate cases — the same bar holds
    _report("disc saturated", g, c["ref"][1], LB.DISC)
    LB.assert_blocks(g, c["ref"][1], LB.DISC, LB.BAR, "disc saturated")


# ---- d. outputs past n stay untouched -------------------------------------------------------------------------------------------------------
def _padded(n, cols, dtype):
    shape = (n + PAD, cols) if cols else (n + PAD,)
    return torch.full(shape, SENTINEL, dtype=dtype, device=DEV)


def _tail_untouched(t, n):
    want = torch.full_like(t[n:], SENTINEL)
    return torch.equal(_bits(t[n:]), _bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("n", LC.ACT_N)
def test_policy_act_at_the_edges_of_its_16_environment_blocks(n):
    c = LC.act_case(n)
    L = A.load()
    w, ob = _dev(c["packed"]), _dev(c["ob"])
    assert w.numel() == L.dm_policy_weight_count()
    outs = []
    for stochastic in (0, 1):
        ac, vp = _padded(n, 28, torch.float64), _padded(n, 0, torch.float32)
        A.check(L.dm_policy_act(_p(w), _p(ob), _p(ac), _p(vp), n, stochastic, 5, 9, _stream()), L)
        torch.cuda.synchronize()
        assert _tail_untouched(ac, n) and _tail_untouched(vp, n)
        outs.append((ac[:n].cpu().numpy(), vp[:n].cpu().numpy()))
    (mean, vp), (sampled, vp_s) = outs
    # means and values against the float64 forward, element by element
    bar = 2e-4 * max(1.0, np.abs(c["mean"]).max())
    print("act n=%d: mean error %.3g, value error %.3g, bar %.3g" % (n, np.abs(mean - c["mean"]).max(), np.abs(vp - c["vpred"]).max(), bar))
    assert np.abs(mean - c["mean"]).max() <= bar
    assert np.abs(vp - c["vpred"]).max() <= min(bar, 2e-4 * max(1.0, np.abs(c["vpred"]).max())) and np.array_equal(vp, vp_s)
    # the draw: (action - mean) / sigma is the counter noise of csrc/rng.h at (seed, counter, env * 28 + action).  Its float32 Box-Muller
    # is within 5.8 (the largest radius of a 24-bit uniform) x ~4e-7 (the float32 rounding of the cosine's argument, up to 2 pi) = 2.5e-6 of
    # the float64 one; rounding mean + sigma eps to float32 adds ~1e-6 / sigma: 1e-5 covers both four times over.
    eps = BN.normal_from(5, 9, np.arange(n * 28, dtype=np.uint64)).reshape(n, 28)
    resid = (sampled - mean) / c["sigma"]
    print("act n=%d: noise error %.3g" % (n, np.abs(resid - eps).max()))
    assert np.abs(resid - eps).max() <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("n", LC.TAIL_N)
def test_pg_losses_writes_old_mean_for_n_rows_only(ppo, n):
    L = A.load()
    D = ppo["D"]
    th = ppo["th"][:LB.NPOL].clone()
    old_mean = _padded(n, 28, torch.float32)
    scratch = torch.empty(int(L.dm_pg_scratch_bytes()), dtype=torch.uint8, device=DEV)
    out = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
    g = torch.full((LB.NPOL,), float("nan"), dtype=torch.float32, device=DEV)
    A.check(L.dm_pg_losses(_p(D["ob"]), n, _p(D["ac"]), _p(D["atarg"]), _p(old_mean), _p(D["old_logstd"]), 1, _p(th), _p(ppo["rms"][0]), _p(ppo["rms"][1]),
                           0.0, 1, _p(g), _p(out), _p(scratch), _stream(), 0), L)
    torch.cuda.synchronize()
    assert _tail_untouched(old_mean, n)
    m, gref = LC.pg_case(n)
    got = old_mean[:n].cpu().numpy()
    assert np.linalg.norm(got - m) <= 1e-5 * np.linalg.norm(m)         # (the existing bar of tests/test_trpo.py)
    _report("pg n=%d" % n, g.cpu().numpy(), gref, LB.POLICY)
    LB.assert_blocks(g.cpu().numpy(), gref, LB.POLICY, LB.BAR, "pg n=%d" % n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", LC.TAIL_N)
def test_disc_reward_writes_n_rows_only(n):
    c = LC.disc_case(33, 31, 1e-3, logit_scale=14.0)
    L = A.load()
    rng = np.random.RandomState(n)
    ob = c["mean"].astype(np.float64) + c["std"] * rng.randn(n, 56) * 1.5
    ac = rng.randn(n, 28) * 0.8
    reward = _padded(n, 0, torch.float64)
    th, mean, std, ob_d, ac_d = (_dev(a) for a in (c["theta"], c["mean"], c["std"], ob, ac))
    A.check(L.dm_disc_reward(_p(th), _p(mean), _p(std), _p(ob_d), _p(ac_d), n, _p(reward), _stream()), L)
    torch.cuda.synchronize()
    assert _tail_untouched(reward, n)
    r = reward[:n].cpu().numpy()
    lg = GN.forward(LC.f64(c["theta"]), c["mean"], c["std"], ob.astype(np.float32), ac.astype(np.float32))[3]
    lo, hi = GN.reward_bracket(lg)
    tol = 1e-5 * np.maximum(1.0, np.abs(hi))
    assert np.isfinite(r).all() and not ((r < lo - tol) | (r > hi + tol)).any(), (r, lo, hi)

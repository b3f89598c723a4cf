"""CPU self-checks of the per-block learner grid's references and cases (tests/learner_blocks.py, tests/vf_numpy.py, tests/learner_cases.py):
the value-fit epoch restatement and the discriminator restatement at entcoeff = 1 against central finite differences of their own losses,
`assert_well_scaled` on every case of tests/test_gpu_learner_edges.py, the constructed PPO minibatches' construction in float64, and the
comparison rule itself (it must fail on an error that the whole-vector bars let through)."""
import numpy as np
import pytest

from tests import gail_numpy as GN
from tests import learner_blocks as LB
from tests import learner_cases as LC
from tests import ppo_numpy as PN
from tests import vf_numpy as VN


def _picks(blocks, rng, per=5):
    return [o + int(k) for _, o, n in blocks for k in rng.choice(n, min(per, n), replace=False)]


def test_block_tables_cover_the_three_layouts():
    assert (LB.NPOL, LB.NVAL, LB.NDISC) == (PN.NPI, PN.NVF, 18701) and VN.NP == LB.NVAL
    for blocks, total in ((LB.POLICY, LB.NPOL), (LB.VALUE, LB.NVAL), (LB.DISC, LB.NDISC), (LB.PPO, LB.NPOL + LB.NVAL)):
        o = 0
        for _, off, n in blocks:                                       # contiguous, in order, no gap
            assert off == o and n > 0
            o += n
        assert o == total
    assert [n for _, _, n in LB.POLICY] == [5600, 100, 10000, 100, 2800, 28, 28]
    assert [n for _, _, n in LB.DISC] == [8400, 100, 10000, 100, 100, 1]


def test_block_rule_catches_what_a_whole_vector_bar_lets_through():
    """The policy's smallest block off by 0.9e-4 of the NET's largest entry: the whole-vector bar does not see it, the block rule does."""
    S = LC.ppo_data()
    ref = LC.ppo_case(33, False)["ref"][1]
    got = ref.copy()
    net = np.abs(ref[:LB.NPOL]).max()
    name, o, n = min(LB.PPO_NETS[0], key=lambda b: np.abs(ref[b[1]:b[1] + b[2]]).max())
    top = np.abs(ref[o:o + n]).max()
    assert top < 0.3 * net
    got[o:o + n] *= 1.0 + 0.9e-4 * net / top                           # a relative error of more than 3e-4 in that block
    assert np.abs(got[:LB.NPOL] - ref[:LB.NPOL]).max() <= 1e-4 * net
    with pytest.raises(AssertionError, match=name):
        LB.assert_blocks(got, ref, LB.PPO)
    LB.assert_blocks(got, ref, LB.PPO, bar={name: 1e-4 * net / top, None: LB.BAR})
    LB.assert_blocks(ref, ref, LB.PPO)
    with pytest.raises(AssertionError, match="1/50"):
        LB.assert_well_scaled(np.concatenate([np.ones(5), [1e-3]]), (("a", 0, 5), ("b", 5, 1)))
    with pytest.raises(AssertionError, match="exempt"):
        LB.assert_well_scaled(np.ones(6), (("a", 0, 5), ("b", 5, 1)), exempt=("b",))
    assert S["first"][0]


def test_value_fit_epoch_gradient_matches_finite_differences():
    c = LC.vf_case(33)
    rec = c["ref"]
    rng = np.random.RandomState(0)
    theta = LC.f64(c["theta0"])
    z, ret = rec[0]["z"], LC.f64(c["ret"][:33])
    g = rec[0]["g"]
    assert np.array_equal(g, VN.gradient(theta, z, ret))
    for i in _picks(LB.VALUE, rng):
        h = 1e-6
        tp, tm = theta.copy(), theta.copy(); tp[i] += h; tm[i] -= h
        fd = (VN.loss(tp, z, ret) - VN.loss(tm, z, ret)) / (2 * h)
        assert abs(fd - g[i]) <= 1e-8 + 1e-5 * abs(g[i]), (i, fd, g[i])
    # the second minibatch saw moved parameters and a moved filter
    assert not np.array_equal(rec[1]["mean"], rec[0]["mean"]) and np.abs(rec[1]["theta"] - rec[0]["theta"]).max() > 1e-5
    # the float32 arithmetic of the same formulas stays close: the envelope the kernels' bars may be set from
    g32 = VN.gradient(c["theta0"], z.astype(np.float32), c["ret"][:33], dtype=np.float32)
    assert g32.dtype == np.float32 and max(LB.block_errors(g32, g, LB.VALUE).values()) < 1e-4


@pytest.mark.parametrize("bs", LC.VF_BS)
def test_value_fit_cases_exercise_the_clip_and_the_floor_and_are_well_scaled(bs):
    c = LC.vf_case(bs)
    for rec in c["ref"]:
        assert (np.abs(rec["z"][:, list(LC.VF_WIDE_COLS)]) == 5.0).any(0).all()          # both wide columns are clipped in some row
        assert rec["std"][LC.VF_CONST_COL] == np.sqrt(np.float32(1e-2))                   # the constant column sits on the floor
        assert (rec["std"] > np.sqrt(np.float32(1e-2))).sum() == 55
        for k in ("g", "m"):
            LB.assert_well_scaled(rec[k], LB.VALUE, what="vf bs=%d %s" % (bs, k))
        top = {name: np.abs(rec["g"][o:o + n]).max() for name, o, n in LB.VALUE}
        for name, o, n in LB.VALUE:                                     # the gradients are most of m and a good part of v: the state carried in hides no error
            assert np.abs(rec["m"][o:o + n]).max() <= 0.3 * top[name] and np.abs(rec["v"][o:o + n]).max() <= 5e-3 * top[name] ** 2
    assert c["rms_after"].count == c["count0"] + 2 * bs


@pytest.mark.parametrize("entcoeff", [1.0])
def test_discriminator_gradient_matches_finite_differences_with_a_large_entropy_term(entcoeff):
    c = LC.disc_case(33, 31, entcoeff)
    theta = LC.f64(c["theta"])
    _, g = c["ref"]
    rng = np.random.RandomState(1)

    def total(th):
        l = LC.disc_reference(c, th)[0]
        return l[0] + l[1] + l[3]                                      # adversary.py total_loss = generator_loss + expert_loss + entropy_loss
    for i in _picks(LB.DISC, rng):
        h = 1e-6
        tp, tm = theta.copy(), theta.copy(); tp[i] += h; tm[i] -= h
        fd = (total(tp) - total(tm)) / (2 * h)
        assert abs(fd - g[i]) <= 1e-8 + 1e-5 * abs(g[i]), (i, fd, g[i])
    # the entropy term is as large as the others: without it the gradient is another one, block by block
    g0 = GN.lossandgrad(theta, *(LC.f64(c[k]) for k in ("mean", "std", "g_ob", "g_ac", "e_ob", "e_ac")), 0.0)[1]
    assert min(LB.block_errors(g0, g, LB.DISC).values()) > 0.05


@pytest.mark.parametrize("entcoeff", LC.DISC_ENT)
@pytest.mark.parametrize("ng,ne", LC.DISC_SHAPES)
def test_discriminator_cases_are_well_scaled(ng, ne, entcoeff):
    c = LC.disc_case(ng, ne, entcoeff)
    LB.assert_well_scaled(c["ref"][1], LB.DISC, what="disc %d,%d ent %g" % (ng, ne, entcoeff))


def test_saturated_discriminator_case_is_saturated():
    c = LC.disc_case(33, 31, 1e-3, logit_scale=14.0)
    lg = GN.forward(LC.f64(c["theta"]), LC.f64(c["mean"]), LC.f64(c["std"]), np.concatenate([c["g_ob"], c["e_ob"]]), np.concatenate([c["g_ac"], c["e_ac"]]))[3]
    assert lg.max() > 17.5 and lg.min() < -17.5 and np.isfinite(c["ref"][0]).all() and np.isfinite(c["ref"][1]).all()
    LB.assert_well_scaled(c["ref"][1], LB.DISC, what="disc saturated")


@pytest.mark.parametrize("gathered", [False, True])
@pytest.mark.parametrize("n", LC.PPO_N)
def test_ppo_cases_are_well_scaled(n, gathered):
    c = LC.ppo_case(n, gathered)
    losses, g = c["ref"]
    for net in LB.PPO_NETS:
        LB.assert_well_scaled(g, net, what="ppo n=%d" % n)
    if n >= 31:
        assert 0 < losses[5] < 1                                       # rows on both sides of the clip
    if gathered and n >= 3:
        _, counts = np.unique(c["rows"][:32], return_counts=True)
        assert counts.max() >= 3                                       # one row three times inside one tile
    if gathered and n > 32:
        assert set(c["rows"][:32]) & set(c["rows"][32:64])             # one row in two tiles


def test_constructed_ppo_minibatches_satisfy_their_construction():
    S = LC.ppo_data()
    c = LC.ppo_constructed("clipped")
    d, clip = c["d"], c["clip"]
    ratio, A = LC.ppo_ratio(S["theta"], S["mean"], S["std"], d), LC.f64(d["atarg"])
    assert ratio.shape == (33,) and (np.abs(ratio - 1.0) > 2 * clip).all() and (np.abs(ratio - 1.0) < 4.0).all()
    assert (np.clip(ratio, 1 - clip, 1 + clip) * A < ratio * A).all()  # the minimum takes the clipped branch on every row
    assert (ratio > 1).any() and (ratio < 1).any()
    losses, g = c["ref"]
    assert losses[5] == 1.0 and not g[:LB.NPOL - 28].any() and np.array_equal(g[LB.NPOL - 28:LB.NPOL], np.full(28, -LC.PPO_ENT))
    LB.assert_well_scaled(g, LB.PPO_NETS[0], exempt=c["zero"])
    LB.assert_well_scaled(g, LB.PPO_NETS[1])
    c = LC.ppo_constructed("zero_adv")
    losses, g = c["ref"]
    assert losses[0] == 0.0 and not g[:LB.NPOL - 28].any() and np.array_equal(g[LB.NPOL - 28:LB.NPOL], np.full(28, -LC.PPO_ENT))
    LB.assert_well_scaled(g, LB.PPO_NETS[0], exempt=c["zero"])
    LB.assert_well_scaled(g, LB.PPO_NETS[1])
    c = LC.ppo_constructed("clip0")
    losses, g = c["ref"]
    assert c["clip"] == 0.0 and losses[5] == 1.0                       # clip = 0: every row is outside the range ...
    assert 0 < (~LC.ppo_rows_first(S["theta"], S["mean"], S["std"], c["d"], 0.0)).sum() < 33          # ... and both branches are taken
    for net in LB.PPO_NETS:
        LB.assert_well_scaled(g, net, what="ppo clip=0")


@pytest.mark.parametrize("n", LC.TAIL_N)
def test_policy_gradient_cases_are_well_scaled(n):
    m, g = LC.pg_case(n)
    assert m.shape == (n, 28)
    LB.assert_well_scaled(g, LB.POLICY, what="pg n=%d" % n)


@pytest.mark.parametrize("n", LC.ACT_N)
def test_policy_act_cases(n):
    c = LC.act_case(n)
    assert c["mean"].shape == (n, 28) and c["vpred"].shape == (n,) and c["packed"].shape == (2 * 56 + LB.NPOL + LB.NVAL,)

"""The parameter blocks of the learner kernels' three flat layouts and the per-block comparison rule — TEST INFRASTRUCTURE.

A gradient check over a whole vector (one norm, one maximum) lets the small blocks hide: the biases, logstd and the value head carry a few
percent of their net's gradient, so an error of a few tenths of a percent in one of them passes a bar of 1e-4 of the net's largest entry.
Those blocks come out of the least obvious parts of the kernels' tile layout (csrc/mlp_tile.h: a bias gradient is "the row after the matrix"
of a weight-gradient tile; csrc/pg_kernel.h: logstd is collected from lanes 0 and 32 of each wave), so every block is held to the bar on its
OWN largest entry.  The offsets below are read from the shapes of the numpy restatements, not from the kernels' headers."""
import numpy as np

from tests import bc_numpy as BN
from tests import gail_numpy as GN
from tests import ppo_numpy as PN

BAR = 1e-4                                                             # the project's bar for these kernels (test_gpu_ppo.py, test_gpu_gail.py)
WELL_SCALED = 1.0 / 50.0


def _blocks(names, shapes):
    out, o = [], 0
    for name, s in zip(names, shapes):
        n = int(np.prod(s))
        out.append((name, o, n)); o += n
    return tuple(out)


POLICY = _blocks(("W1", "b1", "W2", "b2", "W3", "b3", "logstd"), BN.SHAPES)
VALUE = _blocks(("W1", "b1", "W2", "b2", "w3", "b3"), PN.VSHAPES)
DISC = _blocks(("W1", "b1", "W2", "b2", "w3", "b3"), GN.SHAPES)
NPOL, NVAL, NDISC = (sum(n for _, _, n in b) for b in (POLICY, VALUE, DISC))


def shifted(blocks, offset, prefix=""):
    return tuple((prefix + name, o + offset, n) for name, o, n in blocks)


# a PPO theta / gradient: the policy's blocks, then the value net's; one entry per net for assert_well_scaled
PPO_NETS = (shifted(POLICY, 0, "pol/"), shifted(VALUE, NPOL, "vf/"))
PPO = PPO_NETS[0] + PPO_NETS[1]


def _bar_of(bar, name):
    if isinstance(bar, dict):
        return bar.get(name, bar.get(None, BAR))
    return bar


def block_errors(got, ref, blocks):
    """-> {name: max|got_k - ref_k| / max|ref_k|} (inf for a block whose reference is all zero and whose result is not)"""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    out = {}
    for name, o, n in blocks:
        e, s = np.abs(got[o:o + n] - ref[o:o + n]).max(), np.abs(ref[o:o + n]).max()
        out[name] = e / s if s > 0 else (0.0 if e == 0 else np.inf)
    return out


def assert_blocks(got, ref, blocks, bar=BAR, what=""):
    """for every block k: max|got_k - ref_k| <= bar * max|ref_k|.  `bar`: one number, or {block name: bar} (None: the others').  On failure
    every failing block is reported with its worst index (into the flat vector) and both values there."""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s: non-finite entries at %s" % (what, np.flatnonzero(~np.isfinite(got))[:8])
    bad = []
    for name, o, n in blocks:
        err = np.abs(got[o:o + n] - ref[o:o + n])
        scale = np.abs(ref[o:o + n]).max()
        b = _bar_of(bar, name)
        if not err.max() <= b * scale:
            i = o + int(err.argmax())
            bad.append("%s block %s: |%.9g - %.9g| at [%d] = %.3g of the block's largest %.3g (bar %.3g)" % (what, name, got[i], ref[i], i, err.max() / scale if scale > 0 else np.inf, scale, b))
    assert not bad, "\n".join(bad)


def assert_well_scaled(ref, blocks, exempt=(), what=""):
    """The condition that keeps the block rule meaningful, on the reference alone: every block of ONE net has its largest entry at least
    1 / 50 of the net's largest, so a bar on the block's own maximum is not a bar on rounding noise.  `exempt`: blocks that are exactly
    zero by construction (they are asserted to BE zero here; the tests assert exact zeros on the kernel's side)."""
    ref = np.asarray(ref, np.float64).reshape(-1)
    tops = {name: np.abs(ref[o:o + n]).max() for name, o, n in blocks}
    for name in exempt:
        assert tops[name] == 0.0, "%s block %s is exempt as zero by construction but its reference is not zero" % (what, name)
    net = max(tops.values())
    assert net > 0 and np.isfinite(net), what
    for name, top in tops.items():
        if name not in exempt:
            assert top >= WELL_SCALED * net, "%s block %s: largest entry %.3g is %.4f of the net's %.3g (< 1/50): change the case's inputs" % (what, name, top, top / net, net)

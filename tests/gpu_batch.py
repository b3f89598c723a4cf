"""What the GPU tests of a batch share, stated once: the horizon and step buffers, the step / queue / rollout runners, the result dictionaries, the
truncation log, the termination input-condition probe, and the launch forms.  A plain module (no fixtures); it needs torch.  What needs only numpy and a
batch object — STATE, start, state_of, put_state, assert_bits, assert_bits_or_close — lives in tests/helpers.py and is re-exported here.

A new option's test keeps its own make() (the batch configurations differ), its result dictionary and its assertions, names its launch forms as keys of
FORMS (a variant is `FORMS[name]._replace(...)`), and runs them through issue_steps."""
import collections

import numpy as np
import torch

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import MlpPolicy
from tests.helpers import STATE, TERM_FIELDS, assert_bits, assert_bits_or_close, put_state, start, state_of  # noqa: F401  (one import for a test file)

DEV = torch.device("cuda", 0)


# ---- buffers --------------------------------------------------------------------------------------------------------------------------------------
def step_rows(n):
    """one step's outputs (obs, reward, done) on the device"""
    return (torch.zeros((n, 56), dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV))


def horizon_rows(T, n, *, act=None, a0=None):
    """a horizon's buffers -> (ac [T + 1, n, 28], ob [T, n, 56], rew [T, n], dn [T, n] uint8, vp [T, n] float32).  act: the leading action rows (open loop:
    T of them, or all T + 1); a0: row 0 alone (a policy writes the others)"""
    ac = torch.zeros((T + 1, n, 28), dtype=torch.float64, device=DEV)
    if act is not None:
        ac[:len(act)] = torch.as_tensor(act, device=DEV)
    if a0 is not None:
        ac[0] = torch.as_tensor(a0, device=DEV)
    return (ac, torch.zeros((T, n, 56), dtype=torch.float64, device=DEV), torch.zeros((T, n), dtype=torch.float64, device=DEV),
            torch.zeros((T, n), dtype=torch.uint8, device=DEV), torch.zeros((T, n), dtype=torch.float32, device=DEV))


# ---- steps ----------------------------------------------------------------------------------------------------------------------------------------
def step_numpy(b, a, nsub=1, host=False):
    """one finished step -> numpy (obs, rew, done); host: through host pointers"""
    if host:
        o, r, d = b.step(np.ascontiguousarray(a), nsub)
        return o.copy(), r.copy(), d.copy()
    o, r, d = b.step(torch.as_tensor(a, device=DEV), nsub)
    b.join(); b.sync()
    return o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy()


def queued_step(b, a, nsub, keep):
    """dm_batch_step on device buffers of the call's own (what DM_OPT_STEP_QUEUE can queue and DM_OPT_PIPELINE pipeline), kept alive in `keep` as
    (action, obs, reward, done); nothing waits -> the outputs"""
    a = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    out = step_rows(b.n)
    b.step(a, nsub, out)
    keep.append((a,) + out)
    return out


def queued_steps(b, act, t0, t1, nsub=1, keep=None, after=None):
    """steps t0 .. t1 as queued_step calls, then join and sync -> queue_stats seen after every call (after(t) follows it)"""
    keep = [] if keep is None else keep
    seen = []
    for t in range(t0, t1):
        queued_step(b, act[t], nsub, keep)
        seen.append(b.queue_stats())
        if after:
            after(t)
    b.join(); b.sync()
    return seen


# ---- results --------------------------------------------------------------------------------------------------------------------------------------
def result(b, bufs, fields):
    """join, sync -> {"rows<k>": bufs[k] as numpy} and the batch's `fields`"""
    b.join(); b.sync()
    out = {"rows%d" % k: x.cpu().numpy() for k, x in enumerate(bufs)}
    out.update(state_of(b, fields))
    return out


def stacked(b, keep, fields, actions=True):
    """queued_steps' `keep` as result() would give it: rows0 .. 3 = actions, obs, reward, done (without `actions`: rows0 .. 2 = obs, reward, done)"""
    first = 0 if actions else 1
    out = {"rows%d" % (k - first): np.stack([r[k].cpu().numpy() for r in keep]) for k in range(first, 4)}
    out.update(state_of(b, fields))
    return out


def truncation_log(b, *, host=False, device=False, clear=False, cap=None):
    """-> (count, the valid records sorted by (tick, env): index [k, 4], qpos [k, 35], qvel [k, 34]).  host: into host arrays of `cap` rows (the log's size);
    device: device tensors, stream-ordered; neither: what the batch hands out by itself"""
    if host:
        C = b.options[A.OPT_TRUNCATION_LOG] if cap is None else cap
        out = (np.zeros(1, dtype=np.int32), np.zeros((C, 4), dtype=np.int32), np.zeros((C, 35)), np.zeros((C, 34)))
        cnt, idx, qp, qv = b.truncations(clear=clear, out=out)
    elif device:
        cnt, idx, qp, qv = b.truncations(clear=clear, device=True)
        assert cnt.is_cuda and idx.is_cuda and qp.dtype == torch.float64
        b.sync()
    else:
        cnt, idx, qp, qv = b.truncations(clear=clear)
    cnt, idx, qp, qv = ((x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)) for x in (cnt, idx, qp, qv))
    count = int(cnt.reshape(-1)[0])
    k = min(count, idx.shape[0])
    order = np.lexsort((idx[:k, 0], idx[:k, 1]))
    return count, idx[:k][order], qp[:k][order], qv[:k][order]


# ---- the termination input condition ----------------------------------------------------------------------------------------------------------------
def states_before_termination(make_ref, make_probe, idx, q, v, act, nsub):
    """the states the reference's steps leave, ahead of termination: make_ref()'s batch — termination behind step launches — is stepped through `act`, and
    before every step make_probe()'s — the same configuration without termination — takes over its whole state and takes the same step
    -> (qpos [T, n, 35], the step's own done [T, n])"""
    T, n = act.shape[0], len(q)
    ref, probe = make_ref(), make_probe()
    rb, pb = ref.batch, probe.batch
    start(rb, idx, q, v)
    pre_q, stepdone = np.zeros((T, n, 35)), np.zeros((T, n), dtype=bool)
    for t in range(T):
        put_state(pb, state_of(rb))
        a = torch.as_tensor(act[t], device=DEV)
        _o, _r, d = pb.step(a, nsub); pb.join(); pb.sync()
        stepdone[t] = d.cpu().numpy() != 0
        pre_q[t] = pb.get(A.F_QPOS)
        rb.step(a, nsub); rb.join(); rb.sync()
    ref.close(); probe.close()
    return pre_q, stepdone


# ---- launch forms -----------------------------------------------------------------------------------------------------------------------------------
def fused_policy():
    """the policy every fused form runs -> (pol, its packed float32 block); the forms draw with pol._seed and the counters 7, 8, ..."""
    pol = MlpPolicy(device=DEV, seed=2); pol.seed(5)
    return pol, pol.pack()


# packed: DM_OPT_PACKED; pipeline: DM_OPT_PIPELINE; policy: the fused policy step; issue: how the T steps are issued — "step" (dm_batch_step or, with a
# policy, dm_batch_step_act), "rollout" (one dm_batch_rollout call), "queue" (dm_batch_step calls under DM_OPT_STEP_QUEUE = queue_depth; None: 2 T, so that
# nothing launches before the join).  The test's make() applies packed and pipeline; issue_steps the rest.
LaunchForm = collections.namedtuple("LaunchForm", "packed pipeline policy issue queue_depth")
FORMS = {
    "narrow": LaunchForm(0, 1, False, "step", None),                  # k_step_narrow: one env per wave
    "narrow-pipe2": LaunchForm(0, 2, False, "step", None),            # ... as two pipelined sub-batches
    "packed": LaunchForm(1, 1, False, "step", None),                  # k_step_packed + k_step_redo: 33 .. 40 rows go to the redo kernel
    "packed-ext": LaunchForm(2, 1, False, "step", None),              # k_step_packed_ext: the three-set code in the per-step launch
    "narrow-act": LaunchForm(0, 1, True, "step", None),               # dm_batch_step_act
    "packed-act": LaunchForm(1, 1, True, "step", None),
    "rollout": LaunchForm(1, 1, False, "rollout", None),              # dm_batch_rollout without weights
    "rollout-act": LaunchForm(1, 1, True, "rollout", None),           # dm_batch_rollout with weights
    "rollout-narrow-act": LaunchForm(0, 1, True, "rollout", None),
    "queue": LaunchForm(1, 1, False, "queue", None),                  # DM_OPT_STEP_QUEUE: every call queued until the join
    "queue-3": LaunchForm(1, 1, False, "queue", 3),                   # three queued dm_batch_step calls run as one horizon launch
}


def issue_steps(b, form, ac, ob, rew, dn, nsub, *, pol=None, W=None, vp=None, counter=7, between=None):
    """T = len(ob) steps of the batch through `form`, then join and sync.  between(t) follows step t in the forms that issue per step; nothing here joins or
    syncs between steps (a join would turn a queued form into step launches): whether to read state there is the caller's decision."""
    T = int(ob.shape[0])
    if form.issue == "rollout":
        if form.policy:
            b.rollout(ac, (ob, rew, dn), nsub, W, vp, True, pol._seed, counter)
        else:
            b.rollout(ac, (ob, rew, dn), nsub)
    else:
        if form.issue == "queue":
            b.set_option(A.OPT_STEP_QUEUE, form.queue_depth or 2 * T)
        for t in range(T):
            if form.policy:
                b.step_act(ac[t], nsub, (ob[t], rew[t], dn[t]), W, ac[t + 1], vp[t], True, pol._seed, counter + t)
            else:
                b.step(ac[t], nsub, (ob[t], rew[t], dn[t]))
            if between:
                between(t)
    b.join(); b.sync()

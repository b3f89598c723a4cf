"""DeepMimic's early termination (include/dmenv.h DM_OPT_FALL_BODIES / DM_OPT_MAX_EPISODE_STEPS): the named sets of
fall-contact bodies, the parser that turns a set name, body names or body ids into the option's bit mask, and the bits of DM_F_DONE_REASON.

Upstream ends an episode when any body of `--fall_contact_bodies` touches the ground (the lists are in the reference's
src/args/train_humanoid3d_*_args.txt) and after `--time_end_lim_max` seconds.  Here the bodies are the model's (bit b of the mask = model body
b, 1..13, in `CompiledModel.body_names` order), and the time limit is a number of env steps."""
from .humanoid import humanoid_spec

DONE_STEP, DONE_FALL, DONE_TIME_LIMIT = 1, 2, 4      # DM_DONE_*: the step's own done (COM band, clip end) | fall contact | time limit

BODY_NAMES = tuple(b["name"] for b in humanoid_spec()["bodies"])     # [0] is the world

# name -> body names.  "deepmimic": every body except the two ankles (walk, run, the kicks, ...: only the feet may touch the ground);
# "crawl": root, chest and neck (the floor clips: hands, knees and feet carry the humanoid)
FALL_BODY_SETS = {
    "deepmimic": tuple(n for n in BODY_NAMES[1:] if n not in ("right_ankle", "left_ankle")),
    "crawl": ("root", "chest", "neck"),
}


def fall_body_mask(bodies, body_names=BODY_NAMES):
    """DM_OPT_FALL_BODIES for `bodies`: None / "none" / () -> 0 (off); the name of a set in FALL_BODY_SETS; an int (taken as the mask itself);
    or an iterable of body names and / or model body ids (1..13).  ValueError for an unknown name or an id outside 1..13."""
    if bodies is None:
        return 0
    if isinstance(bodies, str):
        if bodies == "none":
            return 0
        if bodies in FALL_BODY_SETS:
            bodies = FALL_BODY_SETS[bodies]
        else:
            bodies = (bodies,)
    elif isinstance(bodies, int):
        if bodies < 0 or bodies & ~(((1 << len(body_names)) - 1) & ~1):
            raise ValueError("fall-body mask %#x: bits 1..%d stand for the model's bodies" % (bodies, len(body_names) - 1))
        return int(bodies)
    mask = 0
    for b in bodies:
        if isinstance(b, str):
            if b not in body_names[1:]:
                raise ValueError("unknown body %r: the model's bodies are %s, the sets %s" % (b, list(body_names[1:]), sorted(FALL_BODY_SETS)))
            b = body_names.index(b)
        b = int(b)
        if not 1 <= b < len(body_names):
            raise ValueError("body id %d outside 1..%d" % (b, len(body_names) - 1))
        mask |= 1 << b
    return mask


def geoms_of_bodies(mask, geom_bodyid):
    """bit g set for every geom g >= 1 of a body in `mask` (what Batch.floor_contacts' bits are tested against)"""
    out = 0
    for g, b in enumerate(geom_bodyid):
        if g >= 1 and (mask >> int(b)) & 1:
            out |= 1 << g
    return out


def reason_names(reason):
    """the set bits of a DM_F_DONE_REASON value by name"""
    return [n for bit, n in ((DONE_STEP, "step"), (DONE_FALL, "fall"), (DONE_TIME_LIMIT, "time_limit")) if int(reason) & bit]

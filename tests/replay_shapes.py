"""The shapes at which the device code between the rollout record and the learner's batch takes another path,
shared by tests/test_replay_shapes_host.py and tests/test_gpu_replay_shapes.py: the replay store at rows and actions wider
than one pass of 256 lanes, the prioritised-replay tree on three levels, the running normalisers with members, chunks and
column tiles at once.  Every function here works on the numpy restatements alone: it states a case's precondition - what makes
the case able to fail - measures it, prints the figures (profiles/pr_replay_shapes.txt keeps them) and asserts it.

  store   K = 256 (D0 = 1282: six passes of j = tid; j < D; j += 256, A = 257: two passes), 6 envs, 5 days, max_days 4 with
          auto-reset (windows end inside the record), capacity 17 (a store of 30 samples is longer than the ring: the first
          13 are skipped; the next store wraps from written = 30)
  tree    capacity 4200: levels 4200, 66, 2, 1; the slots 4096 .. 4199 lie under the second level-2 node
  norm    K = 52 (D = 262: two tiles of 256 columns, the second of 6), members of 7 envs, 150 days: S = 1050 a member, two
          chunks of 1024 samples, the second of 26; 1024 mod 7 = 2: chunk 1 starts inside a day
"""
import numpy as np

from tests import nstep_ref as NS
from tests import per_ref as PR

F = np.float32
LOG = "replay-shapes:"

STORE = dict(K=256, N=6, T=5, C=17, n=3, gamma=0.9)
RESETS = dict(max_days=4, auto_reset=True)
TREE = dict(C=4200, B=300, split=4096, top=256.0)
NORM = dict(K=52, n=7, T=150, cols=(0, 255, 256, 261))
CHUNK, TILE, LANES = 1024, 256, 256


def log(case, **figures):
    print(LOG, case, " ".join(f"{k}={v}" for k, v in figures.items()), flush=True)


# ---- 1. the store -------------------------------------------------------------------------------------------------------------------
def store_windows(case, rec, n, gamma=STORE["gamma"]):
    """the windows of a fetched record [T, N]; asserts that done is mixed, that windows of every length 1 .. n exist (n > 1) and
    that one reaches the fragment's end, where x' is the peeked row"""
    done = np.asarray(rec["terminated"], bool) | np.asarray(rec["truncated"], bool)
    T, N = done.shape
    w = NS.windows(n, gamma, rec["reward"], rec["terminated"], rec["truncated"])
    t = np.repeat(np.arange(T), N)
    reach = t + w["m"] >= T
    lengths = sorted(set(w["m"].tolist()))
    log(case, done=f"{int(done.sum())}/{done.size}", window_lengths=lengths, windows_reaching_the_end=int(reach.sum()),
        rewards_not_zero=int(np.count_nonzero(rec["reward"])))
    assert done.any() and not done.all(), "done was meant to be neither all set nor all clear"
    assert lengths == list(range(1, n + 1)), lengths
    assert reach.any(), "no window reaches the fragment's end: the peeked row is never used"
    return w, reach


def store_columns(case, buf, D, first_store=False):
    """columns 0, 255, 256 and D - 1 of x and x2 differ between at least two slots: a stale or zero tail shows.  After a ring's
    first store nothing stale exists, and a column of x2 may hold one value in every slot if that value is not zero: with two
    frames and windows, every x' the slots of the first store keep is a row of an episode's first or second day, whose older
    frame is the zero row - one normalised constant a column"""
    cols = (0, LANES - 1, LANES, D - 1)
    distinct = {k: [len(set(buf[k][:, c].tolist())) for c in cols] for k in ("x", "x2")}
    log(case, columns=cols, distinct_x=distinct["x"], distinct_x2=distinct["x2"], actions_past_one_pass=int(np.count_nonzero(buf["a"][:, LANES:])))
    assert all(d >= 2 for d in distinct["x"]), distinct
    assert all(d >= 2 or (first_store and buf["x2"][0, c] != 0) for d, c in zip(distinct["x2"], cols)), distinct
    assert np.count_nonzero(buf["a"][:, LANES:]) > 0, "the action's second pass holds zeros only"


def store_peek(case, raw_peek, D0):
    """the peeked raw stacked row [N, H D0] has a nonzero entry at a column at or past 256 of an older frame"""
    older = raw_peek[:, D0 + LANES:]
    log(case, older_frame_entries_past_column_256_not_zero=int(np.count_nonzero(older)))
    assert np.count_nonzero(older) > 0


# ---- 2. the tree ----------------------------------------------------------------------------------------------------------------------
def tree_leaves(seed, size=TREE["C"], split=TREE["split"], lift=20.0):
    """positive leaves spread over three decades, the slots from `split` on raised twentyfold so that they are drawn"""
    rng = np.random.default_rng(seed)
    leaf = 10.0 ** rng.uniform(-2, 1, size)
    leaf[split:] *= lift
    return leaf.astype(F)


def tree_batch(case, idx, split=TREE["split"]):
    """a batch's slots lie on both sides of `split`, hold a duplicate, and hold two different slots under one level-1 node"""
    idx = np.asarray(idx, np.int64)
    low, high = int((idx < split).sum()), int((idx >= split).sum())
    distinct = np.unique(idx)
    dup = idx.size - distinct.size
    nodes = distinct >> 6
    shared = int(nodes.size - np.unique(nodes).size)
    log(case, slots_below_4096=low, slots_from_4096=high, duplicates=dup, slots_sharing_a_level_1_node=shared,
        level_2_nodes=sorted(set((distinct >> 12).tolist())))
    assert low > 0 and high > 0, (low, high)
    assert dup > 0 and shared > 0, (dup, shared)


def tree_shape(capacity=TREE["C"]):
    n = PR.shape(capacity)
    assert n == [4200, 66, 2, 1] or capacity != 4200, n
    return n


# ---- 3. the normalisers -----------------------------------------------------------------------------------------------------------------
def chunk_sizes(S):
    return [min(CHUNK, S - c0) for c0 in range(0, S, CHUNK)]


def norm_shape(case, S, D, n):
    """more than one chunk, more than one column tile, and a second chunk that starts inside a day"""
    chunks, tiles = chunk_sizes(S), [min(TILE, D - c0) for c0 in range(0, D, TILE)]
    log(case, S=S, chunk_sizes=chunks, column_tiles=tiles, chunk_1_starts_at_env=CHUNK % n)
    assert len(chunks) > 1 and len(tiles) > 1 and CHUNK % n != 0
    return chunks


def norm_moved(case, states, start_scales, cols=NORM["cols"]):
    """the members' states differ from one another, and scale differs from its start in the four columns"""
    cols = list(cols)
    moved = [bool(np.all(st["scale"][cols] != s0[cols])) for st, s0 in zip(states, start_scales)]
    differ = all(not np.array_equal(states[a]["mean"], states[b]["mean"]) for a in range(len(states)) for b in range(a))
    log(case, members=len(states), scale_moved_in_the_four_columns=moved, members_differ=differ)
    assert all(moved) and differ

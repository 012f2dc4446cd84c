"""st_ntuple_eval / st_policy_ntuple / st_play_ntuple (TetrisBatch.ntuple_eval,
.policy_ntuple, .play_ntuple) and ntuple.td_update on the device.

The expectation is never the new kernels: it is ntuple_ref (the index and the
chain in numpy; the player composed from the oracle's rows and the boards the
one-env oracle holds after it has locked the piece in a slot), or a composition
of calls other modules hold to the oracle (afterstates, step_placements), or,
for the fused loop, the rounds by hand over policy_ntuple itself, which the
tests above it pin.  Every comparison is bit for bit.

Boards: 10x20 with 70 envs (17.5 workgroups of four envs: the last is partial),
6x9 with 33 (S = 48: lanes past the last slot), 13x12 with 20 (S = 76: two
passes, winners of an earlier pass and -- under a mask -- of the last) and 32x28 with 8 (S = 152: three passes, the
widest LDS rows, a 4x4 tuple in the bottom-right corner).  The states are aged
with policy_greedy (explore 300); AGE is chosen so that the reference rows show
what test_the_sample_exercises_the_paths asserts.  The last two envs are
crafted: one with no valid slot, one whose every valid slot clears two rows.
"""
import ctypes

import numpy as np
import pytest
import torch

import ntuple_ref as NR
import placement_ref as PR
from harness import C4, assert_same_state, cached_ref, engine as _engine, engine_state, pack_cols

pytestmark = pytest.mark.gpu

BOARDS = {"10x20": (10, 20, 70), "6x9": (6, 9, 33), "13x12": (13, 12, 20), "32x28": (32, 28, 8)}
AGE = {"10x20": 400, "6x9": 120, "13x12": 200, "32x28": 900}
NETS = ("3x3", "2x4sm", "mix")
SEED0, ASEED, TABLE_SEED = 9100, 77, 11
DEAD2 = -123.456
GUARD = 64
FILL = {torch.int32: 0x5A5A5A5A, torch.uint8: 0xA5, torch.float32: -7.75, torch.int64: 0x5A5A5A5A5A5A}


def _bits(x):
    x = x if isinstance(x, np.ndarray) else x.cpu().numpy()
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def guarded(shape, dtype, device):
    """(flat, view): a tensor of `shape` with GUARD words of FILL on both sides."""
    numel = int(np.prod(shape))
    flat = torch.full((numel + 2 * GUARD,), FILL[dtype], dtype=dtype, device=device)
    return flat, flat[GUARD:GUARD + numel].view(shape)


def guards_intact(*flats):
    for f in flats:
        fill = torch.tensor(FILL[f.dtype], dtype=f.dtype, device=f.device)
        assert bool((f[:GUARD] == fill).all()) and bool((f[-GUARD:] == fill).all()), "a guard word was written"


def untouched(flat):
    fill = torch.tensor(FILL[flat.dtype], dtype=flat.dtype, device=flat.device)
    return bool((flat == fill).all())


def tuples_of(board, net):
    W, H, _ = BOARDS[board]
    if net == "3x3":
        return NR.systematic(W, H, 3, 3)
    if net == "2x4sm":
        return NR.systematic(W, H, 2, 4, share=True, mirror=True)
    return NR.hand_mix(W, H)


def net_of(board, net):
    G = _engine()
    W, H, _ = BOARDS[board]
    if net == "3x3":
        made = G.NTupleNet.systematic(W, H, 3, 3)
    elif net == "2x4sm":
        made = G.NTupleNet.systematic(W, H, 2, 4, share=True, mirror=True)
    else:
        made = G.NTupleNet(W, H, NR.hand_mix(W, H))
    assert np.array_equal(made.tuples, tuples_of(board, net))
    return made


def kw_of(board, **more):
    W, H, _ = BOARDS[board]
    return dict(width=W, height=H, **C4, **more)


def no_slot_board(W, H):
    """Row 0 full: every piece's anchor cell is occupied wherever it stands."""
    b = np.zeros((W, H), bool)
    b[:, 0] = True
    return b


def two_rows_board(W, H):
    """Row 0 and the two bottom rows filled but for columns 0 and 1: the O fits
    nowhere else, falls to the floor there and completes both rows; what lay in
    row 0 comes down to row 2, so the table sees a compacted board."""
    b = np.zeros((W, H), bool)
    b[2:, 0] = b[2:, H - 2:] = True
    return b


def case(board):
    """The aged and crafted state of a board (a snapshot and get_state's
    arrays) and the reference's rows and boards of it, made once."""
    def make():
        G = _engine()
        W, H, n = BOARDS[board]
        kw = kw_of(board)
        b = G.TetrisBatch(n, autoreset="same_step", seeds=[SEED0 + e for e in range(n)], **kw)
        try:
            b.reset()
            for t in range(AGE[board]):
                b.step(b.policy_greedy(t, seed=ASEED, explore=300), obs="none")
            st = b.get_state(("board", "piece"))
            st["board"][:, n - 2] = pack_cols(no_slot_board(W, H))
            st["board"][:, n - 1] = pack_cols(two_rows_board(W, H))
            st["piece"][n - 1] = (st["piece"][n - 1] & ~np.uint32(7)) | np.uint32(6)  # the O
            b.set_state(**st)
            state = b.get_state(("board", "piece", "stats"))
            snap = b.save()
        finally:
            b.close()
        return dict(snap=snap, state=state, pb=NR.plies_of_state(kw, state), kw=kw)
    return cached_ref(("ntuple_case", board), make)


def indices(board, net):
    return cached_ref(("ntuple_index", board, net), lambda: NR.index_batch(case(board)["pb"], tuples_of(board, net)))


def table_for(board, net):
    return cached_ref(("ntuple_table", board, net),
                      lambda: NR.make_table(NR.table_len(tuples_of(board, net)), TABLE_SEED))


def batch(board, net=None, **more):
    G = _engine()
    _, _, n = BOARDS[board]
    b = G.TetrisBatch(n, autoreset="same_step", seeds=[SEED0 + e for e in range(n)], **kw_of(board, **more))
    b.load(case(board)["snap"])
    if net is not None:
        b.set_ntuple(net_of(board, net))
    return b


# ------------------------------------------------------------------ 0. the sample
@pytest.mark.parametrize("board", sorted(BOARDS))
def test_the_sample_exercises_the_paths(board):
    """On the reference alone: a dead candidate, a slot that clears lines, the
    two crafted envs, and -- with the 3x3 network and three weight rows -- a
    choice other than the linear chain's on at least a quarter of the envs."""
    W, H, n = BOARDS[board]
    pb = case(board)["pb"]
    f = np.stack([p["f"]["base"] for p in pb["plies"]])  # [n, R, S]
    valid = f[:, PR.VALID] != 0
    print("ntuple sample", board, "valid", int(valid.sum()), "dead", int((valid & (f[:, PR.DEAD] != 0)).sum()),
          "clearing", int((valid & (f[:, PR.LINES] > 0)).sum()))
    assert (valid & (f[:, PR.DEAD] != 0)).any(), "no dead candidate"
    assert (valid & (f[:, PR.LINES] > 0)).any(), "no slot clears a line"
    assert not valid[n - 2].any() and valid[n - 1].any() and (f[n - 1, PR.LINES][valid[n - 1]] == 2).all()
    T = len(tuples_of(board, "3x3"))
    for features in ("base", "bcts"):
        w = NR.mixed_weights(3, PR.NF if features == "base" else 18)
        want = NR.score_batch(pb, indices(board, "3x3"), T, table_for(board, "3x3"), w, 0.0, None, features)
        differ = int((want["slots"] != want["s1_slots"]).sum())
        print("ntuple sample", board, features, "choices that differ from S1's", differ, "of", n)
        assert differ * 4 >= n
        assert want["slots"][n - 2] == -1 and want["best"][PR.LINES, n - 1] == 2
    if S_of(board) > 64:  # a winner of an earlier pass than the last: its board is no longer in the lane's LDS row
        last0 = (S_of(board) - 1) // 64 * 64
        early, late = ((want["slots"] >= 0) & (want["slots"] < last0)).sum(), (want["slots"] >= last0).sum()
        print("ntuple sample", board, "winners before the last pass", int(early), "in it", int(late))
        assert early >= 1


def S_of(board):
    return 4 * (BOARDS[board][0] + 6)


# ------------------------------------------------------------------ 1. ntuple_eval
@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("board", sorted(BOARDS))
def test_eval_against_the_reference(board, net):
    """The env boards (read at the state's pitch), 100 caller boards with
    garbage above row H - 1 (m no multiple of 64), one board, and a [W, 3, 5]
    stack: values and indices, either alone, guard words intact."""
    W, H, n = BOARDS[board]
    tuples, tab = tuples_of(board, net), table_for(board, net)
    T = len(tuples)
    b = batch(board, net)
    try:
        dev = b.device
        before = engine_state(b)
        td = torch.as_tensor(tab.copy(), device=dev)
        words = case(board)["state"]["board"].T  # [n, W]
        want_i = NR.index_words(tuples, words)
        assert want_i.min() >= 0 and want_i.max() < len(tab)
        fv, v = guarded((n,), torch.float32, dev)
        fi, ix = guarded((T, n), torch.int32, dev)
        got = b.ntuple_eval(td, out=(v, ix))
        assert got[0] is v and got[1] is ix
        assert np.array_equal(ix.cpu().numpy(), want_i.T)
        assert np.array_equal(_bits(v), _bits(NR.chain(tab, want_i)))
        guards_intact(fv, fi)
        assert torch.equal(b.ntuple_eval(td), v)
        rng = np.random.default_rng(2)
        bools = rng.random((100, W, H)) < rng.uniform(0.1, 0.9, (100, 1, 1))
        bools[0], bools[1] = True, False
        clean = NR.pack(bools)
        dirty = clean | (rng.integers(0, 2 ** 32, clean.shape, dtype=np.uint64).astype(np.uint32)
                         & np.uint32((0xFFFFFFFF << H) & 0xFFFFFFFF))
        want_i = NR.index_words(tuples, clean)
        want_v = NR.chain(tab, want_i)
        for m, shape in ((100, (100,)), (1, (1,)), (15, (3, 5))):
            cb = torch.as_tensor(np.ascontiguousarray(dirty[:m].T).view(np.int32).reshape((W,) + shape), device=dev)
            fv, v = guarded(shape, torch.float32, dev)
            fi, ix = guarded((T,) + shape, torch.int32, dev)
            b.ntuple_eval(td, cb, out=(v, ix))
            assert np.array_equal(ix.cpu().numpy().reshape(T, m), want_i[:m].T), (m, "index")
            assert np.array_equal(_bits(v).reshape(m), _bits(want_v[:m])), (m, "values")
            guards_intact(fv, fi)
            v2, i2 = b.ntuple_eval(td, cb, out=(None, ix.clone()))[1], b.ntuple_eval(td, cb, out=(v.clone(), None))[0]
            assert torch.equal(v2, ix) and torch.equal(i2, v)
        assert_same_state(before, b, "ntuple_eval changed the state")
    finally:
        b.close()


# ------------------------------------------------------------------ 2. policy_ntuple
def run_policy(b, td, w, dv, features, allowed, T):
    n, S, dev = b.n, b.n_slots, b.device
    R = PR.NF if features == "base" else 18
    specs = (((n,), torch.int32), ((n,), torch.uint8), ((n,), torch.float32), ((R, n), torch.int32),
             ((n,), torch.float32), ((T, n), torch.int32), ((n, S), torch.float32))
    flats, views = zip(*(guarded(sh, dt, dev) for sh, dt in specs))
    c = b.policy_ntuple(td, weights=None if w is None else torch.as_tensor(w, device=dev), dead_value=dv,
                        features=features, allowed=None if allowed is None else torch.as_tensor(allowed, device=dev),
                        index=True, values_all=True, out=views)
    guards_intact(*flats)
    return c


def check_choice(c, want, what):
    for name, attr in (("slots", "slots"), ("actions", "actions"), ("best", "feat"), ("index", "index")):
        assert np.array_equal(getattr(c, attr).cpu().numpy(), want[name]), (what, name)
    for name in ("scores", "values", "values_all"):
        assert np.array_equal(_bits(getattr(c, name)), _bits(want[name])), (what, name)


@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("board", sorted(BOARDS))
def test_policy_against_the_reference(board, net):
    """All seven outputs for both feature sets: three weight rows, one row and
    no weights; dead_value 0 and -123.456; without a mask and with one that
    removes the otherwise chosen slot on every second env.  The state stays as
    it was."""
    W, H, n = BOARDS[board]
    S = S_of(board)
    pb, ib, tab = case(board)["pb"], indices(board, net), table_for(board, net)
    T = len(tuples_of(board, net))
    b = batch(board, net)
    try:
        before = engine_state(b)
        td = torch.as_tensor(tab.copy(), device=b.device)
        for features in ("base", "bcts"):
            R = PR.NF if features == "base" else 18
            w3, w1 = NR.mixed_weights(3, R), NR.mixed_weights(1, R, seed=6)
            for w, dv, masked in ((w3, 0.0, False), (w3, DEAD2, True), (w1, DEAD2, False), (None, 0.0, True),
                                  (None, DEAD2, False)):
                what = (features, None if w is None else len(w), dv, masked)
                allowed = None
                if masked:
                    free = NR.score_batch(pb, ib, T, tab, w, dv, None, features)["slots"]
                    allowed = np.ones((n, S), np.int32)
                    for e in range(0, n, 2):
                        if free[e] >= 0:
                            allowed[e, free[e]] = 0
                want = NR.score_batch(pb, ib, T, tab, w, dv, allowed, features)
                if masked:
                    assert (want["slots"][0:n:2] != free[0:n:2]).sum() >= (n - 2) // 2 - 1
                check_choice(run_policy(b, td, w, dv, features, allowed, T), want, what)
        if S > 64:  # only the last pass's slots allowed: the winner's board is still in its lane's LDS row
            last0 = (S - 1) // 64 * 64
            allowed = np.zeros((n, S), np.int32)
            allowed[:, last0:] = 1
            w3 = NR.mixed_weights(3, PR.NF)
            want = NR.score_batch(pb, ib, T, tab, w3, 0.0, allowed, "base")
            assert (want["slots"] >= last0).sum() >= (n - 2) // 2 and (want["index"][0] >= 0).any()
            check_choice(run_policy(b, td, w3, 0.0, "base", allowed, T), want, "the last pass alone")
        # the defaults, and one output alone
        c = b.policy_ntuple(td)
        want = NR.score_batch(pb, ib, T, tab, None, 0.0, None, "base")
        assert c.index is None and c.values_all is None
        assert np.array_equal(c.slots.cpu().numpy(), want["slots"]) and np.array_equal(_bits(c.values), _bits(want["values"]))
        fi, ix = guarded((T, n), torch.int32, b.device)
        b.policy_ntuple(td, index=True, out=(None, None, None, None, None, ix))
        assert np.array_equal(ix.cpu().numpy(), want["index"])
        guards_intact(fi)
        assert_same_state(before, b, "policy_ntuple changed the state")
    finally:
        b.close()


@pytest.mark.parametrize("board", sorted(BOARDS))
def test_values_all_is_eval_of_the_afterstate_boards(board):
    """V of every live candidate is ntuple_eval of afterstates(boards=True)'s
    board of the slot; dead candidates hold dead_value, every other slot 0."""
    net = "2x4sm"
    b = batch(board, net)
    try:
        td = torch.as_tensor(table_for(board, net).copy(), device=b.device)
        a = b.afterstates(boards=True)
        feat = a.feat.cpu().numpy()
        valid, dead = feat[:, PR.VALID] != 0, feat[:, PR.DEAD] != 0
        v = b.ntuple_eval(td, a.boards.permute(1, 0, 2).contiguous()).cpu().numpy()  # [n, S]
        got = b.policy_ntuple(td, dead_value=DEAD2, values_all=True).values_all.cpu().numpy()
        want = np.where(valid & ~dead, v, np.where(valid, np.float32(DEAD2), np.float32(0.0))).astype(np.float32)
        assert (valid & ~dead).sum() > 5 * b.n and (valid & dead).any()
        assert np.array_equal(_bits(got), _bits(want))
    finally:
        b.close()


# ------------------------------------------------------------------ 3. play_ntuple
@pytest.mark.parametrize("features", ["base", "bcts"])
@pytest.mark.parametrize("autoreset", PR.AUTORESETS)
def test_play_equals_the_rounds_by_hand(autoreset, features):
    """10x20, 70 envs, C4 scoring with lock_delay 3: play_ntuple(k = 6) against
    six rounds of policy_ntuple -> step_placements(its slots): sums, last
    outputs and the state; 2 + 4 chained into the caller's tensors; k = 0."""
    G = _engine()
    board, net, K = "10x20", "2x4sm", 6
    W, H, n = BOARDS[board]
    kw = kw_of(board, lock_delay=3)
    seeds = [SEED0 + 500 + e for e in range(n)]
    one, two, twin = (G.TetrisBatch(n, autoreset=autoreset, seeds=seeds, **kw) for _ in range(3))
    try:
        R = PR.NF if features == "base" else 18
        w = torch.as_tensor(NR.mixed_weights(3, R), device=one.device)
        td = torch.as_tensor(table_for(board, net).copy(), device=one.device)
        for x in (one, two, twin):
            x.reset()
            x.play_linear(G.GREEDY_WEIGHTS, 25, placements=True)  # some height before the comparison
            for t in range(60):
                x.step(x.policy_greedy(t, seed=ASEED, explore=300), obs="none")
            x.set_ntuple(net_of(board, net))
        rsum, dsum = np.zeros(n, np.int64), np.zeros(n, np.int32)
        for _ in range(K):
            c = twin.policy_ntuple(td, weights=w, dead_value=DEAD2, features=features)
            last = tuple(x.clone() for x in twin.step_placements(c.slots))
            assert torch.equal(twin.placed != 0, c.slots >= 0)
            rsum += last[1].cpu().numpy()
            dsum += last[2].cpu().numpy()
        print("ntuple play", autoreset, features, "episode ends", int(dsum.sum()), "return", int(rsum.sum()))

        def same(b, ret, eps, what, outs=None):
            o, r, d = outs or (b.obs, b.reward, b.done)
            assert_same_state(b, twin, what)
            assert np.array_equal(ret.cpu().numpy(), rsum) and np.array_equal(eps.cpu().numpy(), dsum), what
            assert torch.equal(o, last[0]) and torch.equal(r, last[1]) and torch.equal(d, last[2]), what

        ret, eps = one.play_ntuple(td, K, weights=w, dead_value=DEAD2, features=features)
        assert ret.dtype == torch.int64 and eps.dtype == torch.int32
        same(one, ret, eps, "k = 6")
        out = (torch.empty_like(two.obs), torch.empty_like(two.reward), torch.empty_like(two.done))
        r2, e2 = two.play_ntuple(td, 2, weights=w, dead_value=DEAD2, features=features, obs="none")
        r2b, e2b = two.play_ntuple(td, 4, weights=w, dead_value=DEAD2, features=features, returns=r2, episodes=e2,
                                   out=out)
        assert r2b is r2 and e2b is e2
        same(two, r2, e2, "k = 2 + 4", out)
        before = (ret.clone(), eps.clone(), one.reward.clone(), one.obs.clone())
        one.play_ntuple(td, 0, weights=w, features=features, returns=ret, episodes=eps)  # k = 0: nothing
        assert_same_state(one, twin, "k = 0")
        assert torch.equal(ret, before[0]) and torch.equal(eps, before[1])
        assert torch.equal(one.reward, before[2]) and torch.equal(one.obs, before[3])
    finally:
        for x in (one, two, twin):
            x.close()


# ------------------------------------------------------------------ 4. td_update
def test_td_update_on_the_device():
    """The dyadic case of test_cpu_ntuple on policy_ntuple's own index: alpha =
    2^-4, integer deltas, a zero table -- exact in any order -- against the
    host loop; envs without a live chosen slot are skipped."""
    G = _engine()
    board, net = "10x20", "2x4sm"
    n = BOARDS[board][2]
    b = batch(board, net)
    try:
        td = torch.as_tensor(table_for(board, net).copy(), device=b.device)
        index = b.policy_ntuple(td, index=True).index
        idx = index.cpu().numpy()
        assert (idx[0] < 0).any() and (idx[0] >= 0).sum() > n // 2 and ((idx >= 0).all(axis=0) | (idx < 0).all(axis=0)).all()
        delta = np.random.default_rng(3).integers(-20, 21, n).astype(np.float32)
        want = np.zeros(len(td), np.float64)
        for t in range(idx.shape[0]):
            for e in range(n):
                if idx[0, e] >= 0:
                    want[idx[t, e]] += 2.0 ** -4 * delta[e]
        table = b._ntuple.new_table(b.device)
        assert table.shape == td.shape and not table.any()
        out = G.td_update(table, index, torch.as_tensor(delta, device=b.device), 2.0 ** -4)
        assert out is table and table.is_cuda
        assert np.array_equal(table.cpu().numpy(), want.astype(np.float32))
        assert (want != 0).sum() > 50
    finally:
        b.close()


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_state_and_outputs_alone():
    G = _engine()
    from gym_simpletetris_amd import _lib as C
    board, net = "6x9", "mix"
    n = BOARDS[board][2]
    b = batch(board)
    try:
        dev = b.device
        before = engine_state(b)
        tab = table_for(board, net)
        td = torch.as_tensor(tab.copy(), device=dev)
        fs, sl = guarded((n,), torch.int32, dev)
        fr, ret = guarded((n,), torch.int64, dev)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        L = b._L
        # no network set: the host layer, and the library itself
        for call in (lambda: b.policy_ntuple(td), lambda: b.play_ntuple(td, 1), lambda: b.ntuple_eval(td)):
            with pytest.raises(RuntimeError, match="set_ntuple"):
                call()
        assert L.st_policy_ntuple(b._ctx, 0, None, 0, p(td), 0.0, None, p(sl), None, None, None, None, None, None,
                                  None) == C.ST_ESTATE
        assert L.st_play_ntuple(b._ctx, 0, None, 0, p(td), 0.0, 1, p(ret), None, None, None, None, None) == C.ST_ESTATE
        assert L.st_ntuple_eval(b._ctx, p(td), None, 0, p(sl), None, None) == C.ST_ESTATE
        assert b"network" in L.st_last_error()
        # a malformed network changes nothing
        bad = np.array([[0, 0, 3, 3, 0, 0], [4, 0, 3, 3, 0, 0]], np.int32)  # columns 4..6 of a 6-wide board
        assert L.st_ntuple_set(b._ctx, bad.ctypes.data_as(ctypes.c_void_p), 2) == C.ST_EINVAL
        assert b"tuple 1" in L.st_last_error() and L.st_ntuple_table_len(b._ctx) == 0
        b.set_ntuple(net_of(board, net))
        assert L.st_ntuple_table_len(b._ctx) == len(tab)
        assert L.st_ntuple_set(b._ctx, bad.ctypes.data_as(ctypes.c_void_p), 2) == C.ST_EINVAL
        assert L.st_ntuple_table_len(b._ctx) == len(tab)
        # a table too short (host layer), a non-finite dead_value (host layer and library)
        for call in (lambda: b.policy_ntuple(td[:-1].contiguous(), out=(sl, None, None, None, None)),
                     lambda: b.play_ntuple(td[:-1].contiguous(), 1), lambda: b.ntuple_eval(td[:-1].contiguous())):
            with pytest.raises(ValueError, match="table"):
                call()
        for bad_dv in (float("inf"), float("nan")):
            with pytest.raises(ValueError, match="dead_value"):
                b.policy_ntuple(td, dead_value=bad_dv, out=(sl, None, None, None, None))
            with pytest.raises(ValueError, match="dead_value"):
                b.play_ntuple(td, 1, dead_value=bad_dv, returns=ret)
            assert L.st_policy_ntuple(b._ctx, 0, None, 0, p(td), bad_dv, None, p(sl), None, None, None, None, None,
                                      None, None) == C.ST_EINVAL
            assert L.st_play_ntuple(b._ctx, 0, None, 0, p(td), bad_dv, 1, p(ret), None, None, None, None,
                                    None) == C.ST_EINVAL
        assert L.st_policy_ntuple(b._ctx, 0, None, 0, p(td), 0.0, None, None, None, None, None, None, None, None,
                                  None) == C.ST_EINVAL
        torch.cuda.synchronize()
        assert untouched(fs) and untouched(fr)
        assert_same_state(before, b, "a refused call changed the state")
        # the network is still the one set: removing it brings the first refusal back
        want = NR.score_batch(case(board)["pb"], indices(board, net), len(tuples_of(board, net)), tab, None, 0.0)
        assert np.array_equal(b.policy_ntuple(td).slots.cpu().numpy(), want["slots"])
        b.set_ntuple(None)
        with pytest.raises(RuntimeError, match="set_ntuple"):
            b.policy_ntuple(td)
    finally:
        b.close()

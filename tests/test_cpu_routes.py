"""Routes without a GPU: the packed encoding, and route_ref's walked route
against the header's definition taken literally (reach_ref.search's lowest
first action, one oracle step, and again) on a few envs of three samples."""
import numpy as np
import pytest

import reach_ref as R
import route_ref as RR
from harness import cached_ref

CASES = [("10x20", "default"), ("6x9", "lock2"), ("11x12", "c4_lock3")]
ENVS = (0, 23, 46, 69)  # young to old boards of the aged sample


def test_pack_unpack_round_trip():
    from gym_simpletetris_amd import _lib as C
    from gym_simpletetris_amd.engine import route_pack, route_unpack
    assert (C.ROUTE_MAX, C.ROUTE_WORDS) == (RR.ROUTE_MAX, RR.ROUTE_WORDS) == (42, 2)
    rng = np.random.default_rng(5)
    for n in (0, 1, 20, 21, 22, 41, 42):
        acts = rng.integers(0, 7, n).tolist()
        w = route_pack(acts)
        assert w.dtype == np.uint64 and w.shape == (2,)
        assert [int(x) for x in w] == RR.pack(acts)
        assert all(int(x) >> 63 == 0 for x in w), "bit 63"
        fields = [(int(w[i // 21]) >> (3 * (i % 21))) & 7 for i in range(42)]
        assert fields[:n] == acts and all(f == 7 for f in fields[n:]), "the fill behind the route is 7"
        assert route_unpack(w) == acts
        assert route_unpack(w.view(np.int64)) == acts  # as a Routes holds the words
    assert [int(x) for x in route_pack([])] == [(1 << 63) - 1] * 2
    for bad in ([7], [-1], [0] * 43):
        with pytest.raises(ValueError):
            route_pack(bad)


def _routes_of(board, config):
    def make():
        smp, kw = R.sample(board, config), R.case_kw(board, config)
        h, hf = R.helpers(kw)
        out = []
        for e in ENVS:
            er = RR.env_routes(h, hf, smp["ob"], e)
            assert np.array_equal(er.steps(), smp["steps"][e]), ("distances", e)
            out.append((e, er, {int(s): er.route(int(s)) for s in range(-1, len(er.valid) + 1)}))
        return out
    return cached_ref(("cpu_routes", board, config), make)


@pytest.mark.parametrize("board,config", CASES)
def test_walked_route_is_the_iterated_first_action(board, config):
    smp, kw = R.sample(board, config), R.case_kw(board, config)
    h, hf = R.helpers(kw)
    longest = 0
    for e, er, routes in _routes_of(board, config):
        env = smp["ob"].envs[e]
        steps = smp["steps"][e]
        for s, acts in routes.items():
            served = 0 <= s < len(steps) and steps[s] > 0
            assert len(acts) == (steps[s] if served else 0), (e, s)
            longest = max(longest, len(acts))
        # the definition, literally, and the replay through the oracle: it locks at the landing on step n, not before
        reach = np.flatnonzero(steps)
        for s in reach[:: max(1, len(reach) // 6)]:
            lit, where = RR.iterate_first(h, hf, smp["ob"].board(e), env.shape_id, env.rot, env.ax, env.ay, env.lock,
                                          int(s), smp["Y"][e, s])
            assert lit == routes[int(s)], (e, s, lit, routes[int(s)])
            assert where == er.target(int(s)), (e, s)
            h.load(smp["ob"].board(e), env.shape_id)
            st = (env.rot, env.ax, env.ay, env.lock)
            for i, a in enumerate(lit):
                *st, locked, _ = h.step(*st, a)
                assert locked == (i == len(lit) - 1), ("locks on step n and not before", e, s, i)
    print(f"longest route on {board} / {config}: {longest}")
    assert longest <= RR.ROUTE_MAX


def test_longest_route_fits_the_words():
    """Every sample of reach_ref, every env, every slot: the longest shortest
    route (st_reachable's steps) stays within ROUTE_MAX."""
    longest = max(int(R.sample(b, c)["steps"].max()) for b, c in R.CASES)
    print(f"longest route over all samples: {longest}")
    assert 0 < longest <= RR.ROUTE_MAX

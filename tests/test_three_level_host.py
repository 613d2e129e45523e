"""Host logic of the three-level launches: the schedule rewrite (group_triples).  No GPU."""
from feanet_amd.schedule import (OMDF, group_triples, pair_prolongations, pair_restrictions, vcycle_schedule)


def kinds(steps):
    return [(st[0], st[1]) for st in steps]


def grouped(L, tail_from, down=True, up=True, **kw):
    steps, end = vcycle_schedule(L, tail_from=tail_from, **kw)
    steps = group_triples(steps, lambda l: down, lambda l: up)
    return pair_prolongations(pair_restrictions(steps, lambda l: True), lambda l: True), end


def test_metric_cycle_groups_the_three_levels_above_the_tail():
    """4097^2: levels 1 .. 5 above the tail (level 6): the last three go to the three-level steps, 1-2 pair."""
    steps, end = grouped(12, 6)
    assert kinds(steps) == [("sweep_restrict", 0), ("resid_restrict2", 1), ("resid_restrict3", 3), ("coarse_tail", 6),
                            ("prolong_sweep3", 3), ("prolong_sweep2", 1), ("prolong_sweep", 0)]
    tail, up3, up2, top = steps[3], steps[4], steps[5], steps[6]
    assert up3 == ("prolong_sweep3", 3, tail[2], "a")      # reads the tail's output, writes level 3's iterate
    assert up2[2] == up3[3] and top[3] == up2[3] and end == top[4]


def test_three_levels_alone():
    """1025^2 (C2): levels 1 .. 3, then the tail."""
    steps, _ = grouped(10, 4)
    assert kinds(steps) == [("sweep_restrict", 0), ("resid_restrict3", 1), ("coarse_tail", 4), ("prolong_sweep3", 1),
                            ("prolong_sweep", 0)]


def test_even_runs_are_left_to_the_pairs():
    """Two or four levels above the tail pair up already: a triple would not save a launch."""
    for L, t in ((9, 3), (11, 5)):
        steps, _ = grouped(L, t)
        assert not any(st[0] in ("resid_restrict3", "prolong_sweep3") for st in steps), steps
    steps, _ = grouped(11, 5)
    assert kinds(steps) == [("sweep_restrict", 0), ("resid_restrict2", 1), ("resid_restrict2", 3), ("coarse_tail", 5),
                            ("prolong_sweep2", 3), ("prolong_sweep2", 1), ("prolong_sweep", 0)]


def test_each_direction_has_its_own_switch():
    steps, _ = grouped(10, 4, up=False)
    assert kinds(steps) == [("sweep_restrict", 0), ("resid_restrict3", 1), ("coarse_tail", 4), ("prolong_sweep", 3),
                            ("prolong_sweep2", 1), ("prolong_sweep", 0)]
    steps, _ = grouped(10, 4, down=False)
    assert kinds(steps) == [("sweep_restrict", 0), ("resid_restrict2", 1), ("resid_restrict", 3), ("coarse_tail", 4),
                            ("prolong_sweep3", 1), ("prolong_sweep", 0)]


def test_other_cycles_are_left_alone():
    """Stored iterates (V(2,2)), no post-sweep, the q2 compatibility mode and a cycle without a tail have no run of
    zero-guess restrictions / recomputed prolongations at the tail: nothing is rewritten."""
    for kw in (dict(nu1=2, nu2=2), dict(nu2=0), dict(compat="mm_interface_q2")):
        steps, _ = vcycle_schedule(10, tail_from=4, **kw)
        assert group_triples(steps, lambda l: True, lambda l: True) == steps, kw
    steps, _ = vcycle_schedule(10)
    assert group_triples(steps, lambda l: True, lambda l: True) == steps
    steps, _ = vcycle_schedule(10, tail_from=4)
    assert ("prolong_sweep", 3, OMDF, "a", "a") in steps     # what the rewrite looks for

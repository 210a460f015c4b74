"""The designs of tests/test_gpu_gather_walk.py without a GPU: each meets the partition it states, its members' chunks are the sizes its name
says, and the fp64 oracle alone is finite on it at the three points of the comparison."""
import numpy as np
import pytest

from test_gpu_cluster_builds import assert_preconditions
from test_gpu_gather_walk import WALK, reference

CHUNKS = 8


def chunk_sizes(polls):
    return [polls * (w + 1) // CHUNKS - polls * w // CHUNKS for w in range(CHUNKS)]


@pytest.mark.parametrize("name", list(WALK))
def test_design_meets_its_partition_and_the_oracle_is_finite(name):
    dz, q, lpg = reference(name)
    mem = assert_preconditions(dz)
    assert len(q) == 3
    for lp, g in lpg:
        assert np.isfinite(lp) and np.isfinite(g).all() and np.abs(g).max() > 0
    sizes = {c for polls, _, _ in mem for c in chunk_sizes(polls)}
    kind, _, what = name.partition("/")
    if what.endswith("_polls") and what[:-6].isdigit():
        assert sizes == {int(what[:-6])}, sizes
        assert (dz["tag"] >= 16) == (kind == "fixed")
    expect = {"chunk/empty_chunks": {0, 1}, "days/no_polls_and_one_day_with_all": {0, 12, 13}, "days/ends_at_group_edges": {24}, "chunk/second_trip_tag8": {80}}
    if name in expect:
        assert sizes == expect[name], sizes


def test_day_ends_sit_on_both_sides_of_the_group_edges():
    """days/ends_at_group_edges: in the first chunk of every member a day ends on slots 7, 8, 15, 16 and 23 (the chunk's last)."""
    dz = WALK["days/ends_at_group_edges"]()
    data = dz["data"]
    day = np.sort(np.concatenate([data["day_state"], data["day_national"]]).astype(int))
    for m in range(dz["K"]):
        own = day[(day > 8 * m) & (day <= 8 * m + 8)]
        assert len(own) == 192
        ends = [i for i in range(24) if own[i + 1] != own[i]]
        assert ends == [7, 8, 15, 16, 23], ends

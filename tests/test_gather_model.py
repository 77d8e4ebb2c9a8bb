"""tests/gather_model.py pinned on the CPU: list indexing and the null-pick rules of pvac_hip_batch_gather."""
import pytest

import gather_model as gm


def test_picks_index_the_sources():
    A, B = ["a0", "a1", "a2"], ["b0"]
    assert gm.gather([A, B], [1, 0, 0, 0], [0, 2, 2, 0]) == ["b0", "a2", "a2", "a0"]   # repeats, any order
    assert gm.gather([A, B, []], [0], [1]) == ["a1"]                                   # a source may go unused
    assert gm.gather([A, B], [], []) == []


def test_null_pick_rules():
    A, B = ["a0", "a1"], ["b0"]
    assert gm.gather([A, [], B]) == ["a0", "a1", "b0"]          # no picks: the concatenation
    assert gm.gather([]) == []
    assert gm.gather([A], None, [1, 1, 0]) == ["a1", "a1", "a0"]   # pick_src null: the one source
    for bad in (lambda: gm.gather([A, B], None, [0]),              # ... and only one
                lambda: gm.gather([], None, [0]),
                lambda: gm.gather([A, B], [0], None),              # pick_src needs pick_idx
                lambda: gm.gather([], [0], [0]),                   # ciphers without a source
                lambda: gm.gather([A, B], [2], [0]),               # pick_src out of range
                lambda: gm.gather([A, B], [1], [1]),               # pick_idx out of range for its source
                lambda: gm.gather([[]] * (gm.MAX_SOURCES + 1))):
        with pytest.raises(gm.GatherError) as e:
            bad()
        assert e.value.code == gm.EINVAL


def test_split_inverts_concatenation():
    xs = [["a", "b"], [], ["c"]]
    assert gm.split(gm.gather(xs), [2, 0, 1]) == xs

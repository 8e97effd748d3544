"""CPU: ``plan.lru``, the one "keep the N most recent" cache behind the backbones' plans, the neck's launch states and the head modules' replay states."""
from toc3d_amd.plan import lru


def test_hit_reorders_and_does_not_make():
    cache, made = {}, []

    def make(v):
        return lambda: made.append(v) or v
    for k in "abc":
        assert lru(cache, k, make(k.upper()), 3) == k.upper()
    assert list(cache) == ["a", "b", "c"] and made == ["A", "B", "C"]
    assert lru(cache, "a", make("never"), 3) == "A", "a hit returns what is stored"
    assert list(cache) == ["b", "c", "a"] and made == ["A", "B", "C"], "the hit moved to the end; make was not called"
    assert lru(cache, "a", make("never"), 1) == "A" and len(cache) == 3, "a hit evicts nothing, whatever the bound"


def test_miss_evicts_oldest_first_before_it_makes():
    cache = {k: k for k in range(6)}
    lru(cache, 2, None, 4)                                                # (a hit: 2 is now the most recent)
    seen = []
    assert lru(cache, "new", lambda: seen.append(list(cache)) or "made", 4) == "made"
    assert seen == [[4, 5, 2]], "down to keep - 1 entries, oldest first, before make() runs"
    assert list(cache.items()) == [(4, 4), (5, 5), (2, 2), ("new", "made")]
    lru(cache, "next", dict, 4)
    assert list(cache) == [5, 2, "new", "next"]


def test_keep_none_never_evicts():
    cache = {}
    for k in range(100):
        lru(cache, k, dict)
    assert list(cache) == list(range(100))
    lru(cache, 0, dict, None)
    assert list(cache) == list(range(1, 100)) + [0]

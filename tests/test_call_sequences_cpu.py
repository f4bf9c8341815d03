"""The call-sequence harness without a GPU (tests/call_sequences.py): the generator reaches every ordered pair of op kinds, and replay()
catches planted errors of the three kinds it exists for -- on a numpy stand-in context with the surface of the library's (snapshot / load) and
a cache flag: a writer that forgets to drop the cache, a no-op kind that changes a field, a returned array that depends on history."""
import numpy as np
import pytest

import call_sequences as cs


# ---- the generator ----
def test_every_ordered_pair_of_kinds_is_adjacent_somewhere():
    seqs = cs.sequences()
    m = cs.pair_coverage(seqs.values())
    assert m.shape == (len(cs.KINDS), len(cs.KINDS))
    missing = [(cs.KINDS[a], cs.KINDS[b]) for a, b in np.argwhere(m == 0)]
    assert not missing, missing
    # the matrix counts what the sequences hold, pair by pair
    assert m.sum() == sum(len(s) - 1 for s in seqs.values())
    assert m[cs.KINDS.index("P"), cs.KINDS.index("S")] >= 1 and cs.pair_coverage([("P", "S")]).sum() == 1


def test_every_kind_occurs_and_has_an_op():
    seqs = cs.sequences()
    seen = {k for s in seqs.values() for k in s}
    assert seen == set(cs.KINDS) == set(cs.OPS)
    assert set(cs.NOOP_KINDS) <= set(cs.KINDS)
    assert all(set(s) <= set(cs.KINDS) and len(s) >= 2 for s in seqs.values())
    # the hand-written list stays in, under its names, in front of the random ones
    assert list(seqs)[:len(cs.HAND)] == list(cs.HAND) and all(seqs[k] == tuple(v) for k, v in cs.HAND.items())
    rnd = [k for k in seqs if k.startswith("random-")]
    assert rnd and all(len(seqs[k]) == 20 for k in rnd)
    # the pairs the issue names
    pairs = set().union(*(cs.pairs_of(s) for s in cs.HAND.values()))
    for p in (("P", "S"), ("Q", "C"), ("F", "S"), ("VD", "C"), ("C", "I"), ("I", "S"), ("S0", "C"), ("RV", "S"), ("H", "C"), ("C", "H"), ("S", "P1"),
              ("C", "P1")):
        assert p in pairs, p


def test_the_sequences_are_deterministic():
    a = dict(cs.sequences())
    cs.sequences.cache_clear()
    b = dict(cs.sequences())
    assert list(a) == list(b) and a == b
    covered = set()
    assert cs._random_sequence(3, covered) == cs._random_sequence(3, set())
    assert cs._random_sequence(3, set()) != cs._random_sequence(4, set())


# ---- the stand-in context ----
class Standin:
    """state: x[4][3] and y[4]; hidden: a cached column sum of x (valid flag), a call counter.  Ops:
       step   x <- 0.5 * x + (column sums of x, cached or formed afresh) + y; leaves the sums of the new x cached
       put    writes x with its own bits (no visible change): must drop the cache
       scale  y <- 2 * y (x is untouched, the cache stays valid)
       peek   a no-op kind: returns the column sums formed afresh
       get    returns x + y[:, None]
    bug: "put_keeps_cache" | "peek_writes" | "get_counts" | None"""
    count = 0

    def __init__(self, bug=None):
        self.bug = bug
        self.x = np.zeros((4, 3)); self.y = np.zeros(4)
        self.sums, self.valid, self.calls, self.tag = np.zeros(3), False, 0, 0
        Standin.count += 1

    def field_names(self):
        return ("x", "y")

    def read(self, name):
        return getattr(self, name).copy()

    def write(self, name, a):
        getattr(self, name)[...] = a

    def scalars(self):
        return dict(tag=self.tag)

    def set_scalars(self, s):
        self.tag = s["tag"]

    def invalidate_cache(self):
        self.valid = False

    def dcmip_init(self):
        pass

    def start(self):
        self.x[...] = np.arange(12.0).reshape(4, 3) / 7.0
        self.y[...] = [0.1, 0.2, 0.3, 0.4]

    def close(self):
        self.closed = True


def _step(c):
    c.calls += 1
    s = c.sums if c.valid else c.x.sum(axis=0)
    c.x[...] = 0.5 * c.x + s[None, :] + c.y[:, None]
    c.sums, c.valid = c.x.sum(axis=0), True
    c.tag += 1


def _put(c):
    c.calls += 1
    c.x[...] = c.x.copy() * 1.0
    c.sums = c.sums + 1.0            # what a cache that was not refreshed is worth: it only shows if it is used
    if c.bug != "put_keeps_cache":
        c.valid = False


def _scale(c):
    c.calls += 1
    c.y *= 2.0


def _peek(c):
    c.calls += 1
    if c.bug == "peek_writes":
        c.y[2] = np.nextafter(c.y[2], 1.0)      # one unit in the last place of one entry
    return dict(sums=c.x.sum(axis=0))


def _get(c):
    c.calls += 1
    out = c.x + c.y[:, None]
    if c.bug == "get_counts" and c.calls > 3:
        out[1, 2] = -out[1, 2]
    return dict(field=out, n=7)


OPS = dict(S=_step, VQ=_put, H=_scale, M=_peek, G=_get)   # under kinds of the vocabulary: VQ and M are no-op kinds there
SEQ = ("S", "VQ", "S", "H", "M", "G", "S", "M", "VQ", "G", "S")


def test_the_stand_in_passes_without_a_bug():
    Standin.count = 0
    kept = cs.replay(lambda: Standin(), SEQ, OPS, keep=True)
    assert Standin.count == 1 + len(SEQ)                     # one warm context and a fresh one per op
    assert len(kept) == len(SEQ) and kept[-1][0]["scalars"] == dict(tag=4)
    assert sorted(kept[5][1]) == ["field", "n"] and kept[0][1] == {}


def test_a_writer_that_forgets_to_drop_the_cache_is_caught():
    with pytest.raises(cs.SequenceMismatch) as ei:
        cs.replay(lambda: Standin("put_keeps_cache"), SEQ, OPS)
    e = ei.value
    # the put itself leaves the same bits; the step behind it runs on the stale cache
    assert (e.what, e.field, e.index, e.kind, e.prev) == ("state", "x", 2, "S", "VQ"), str(e)
    assert e.where == (0, 0) and "op 2 (S) after VQ" in str(e) and "x" in str(e)


def test_a_no_op_kind_that_changes_a_field_is_caught():
    with pytest.raises(cs.SequenceMismatch) as ei:
        cs.replay(lambda: Standin("peek_writes"), SEQ, OPS)
    e = ei.value
    assert (e.what, e.field, e.index, e.kind, e.prev) == ("noop", "y", 4, "M", "H"), str(e)
    assert e.where == (2,) and "1 of 4 entries differ" in str(e)


def test_a_returned_array_that_depends_on_history_is_caught():
    with pytest.raises(cs.SequenceMismatch) as ei:
        cs.replay(lambda: Standin("get_counts"), SEQ, OPS)
    e = ei.value
    assert (e.what, e.field, e.index, e.kind, e.prev) == ("returned", "field", 5, "G", "M"), str(e)
    assert e.where == (1, 2)


def test_bits_not_values_are_compared():
    """a NaN equals itself bit for bit, two NaNs of different payload do not, and -0.0 is not +0.0"""
    nan_a = np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)
    nan_b = np.array([0x7FF8000000000002], dtype=np.uint64).view(np.float64)
    assert cs._first_difference(cs.bits(nan_a), cs.bits(nan_a.copy())) is None
    assert cs._first_difference(cs.bits(nan_a), cs.bits(nan_b))[0] == (0,)
    assert cs._first_difference(cs.bits(np.array([0.0])), cs.bits(np.array([-0.0])))[0] == (0,)
    assert cs._first_difference(cs.bits(np.zeros(3)), cs.bits(np.zeros(4)))[0] == ()


def test_snapshot_and_load_round_trip():
    a = Standin(); a.start(); _step(a)
    s = cs.snapshot(a)
    b = Standin(); b.valid = True
    cs.load(b, s)
    assert not b.valid and b.tag == 1
    t = cs.snapshot(b)
    assert all(np.array_equal(s["fields"][k], t["fields"][k]) for k in ("x", "y")) and s["scalars"] == t["scalars"]
    a.x[0, 0] = 5.0
    assert s["fields"]["x"][0, 0] != cs.bits(a.x)[0, 0]      # a snapshot is a copy

"""The helpers of tests/wideband_options.py on fake handles, without the library: every assertion of every helper fires on a handle
that breaks it, and none on handles that keep it."""
import numpy as np
import pytest

import wideband_options as wo

LEVELS = np.dtype([("sum_sq", np.int64), ("clipped", np.int32), ("gain", np.float32)])
RECORDS = np.dtype([("channel", np.int32), ("item", np.int32), ("message", np.uint8, 10)])
FAILS = (AssertionError, pytest.fail.Exception)            # pytest.raises inside code_of fails in its own way when nothing is raised


class Fake:
    """Two channels; what it reports after push i is made of i and of the part pushed, so that two fakes fed the same parts agree.
    `bend`: {what: push} - what to report differently at that push."""

    channels = 2

    def __init__(self, bend=(), silent=False):
        self.bend, self.silent, self.i, self.closed = dict(bend), silent, -1, False

    def _bent(self, what):
        return self.bend.get(what) == self.i

    def push_wideband(self, slot, part, first=False):
        assert slot == (self.i + 1) % 2 or first
        self.i = 0 if first else self.i + 1
        self.part = np.asarray(part)

    def dump_wideband_hop(self, c):
        hop = np.zeros((4, 2), dtype=np.int8) if self.silent else (self.part[:8] + c).astype(np.int8).reshape(4, 2)
        if c == 1 and self._bent("hops"):
            hop[3, 1] ^= 1
        return hop

    def wideband_clip_count(self):
        return 7 + self.i + self._bent("clip")

    def wideband_levels(self):
        out = np.zeros(self.channels, dtype=LEVELS)
        out["sum_sq"], out["clipped"], out["gain"] = 1000 + self.i, 3, 2.5
        if self._bent("levels"):
            out["gain"][1] = np.nextafter(np.float32(2.5), np.float32(3))
        return out

    def extra(self):
        power = np.arange(4, dtype=np.float64) * (0 if self.silent else self.i + 1)
        if self._bent("extra"):
            power[2] = -power[2]
        return power, 0 if self.silent else 5

    def decode(self):
        pass

    def fetch_async(self, s):
        pass

    def fetch_wait(self, s):
        r = np.zeros(2, dtype=RECORDS)
        r["channel"], r["item"], r["message"][:, 0] = [1, 0], [4, 9], self.i + 1
        if self._bent("records"):
            r["message"][1, 9] = 1
        return r, None

    def close(self):
        self.closed = True


PARTS = [np.arange(1, 17, dtype=np.int16) * k for k in (1, 2, 3)]


def test_leaves_unchanged_passes_when_the_handles_agree_and_returns_what_it_saw():
    seen = wo.leaves_unchanged(Fake(), Fake(), PARTS, reads=(Fake.extra,), decode=True)
    assert len(seen) == 3 and [s["clip"] for s in seen] == [7, 8, 9]
    assert seen[1]["hops"].shape == (2, 4, 2) and seen[2]["reads"][0][1] == 5 and seen[2]["levels"]["sum_sq"][0] == 1002
    assert list(seen[0]["records"]["channel"]) == [0, 1]                # sorted, as wideband_gpu._decode leaves them
    assert "records" not in wo.leaves_unchanged(Fake(), Fake(), PARTS)[0]


@pytest.mark.parametrize("what", ["hops", "clip", "levels", "extra", "records"])
@pytest.mark.parametrize("push", [0, 2])
def test_leaves_unchanged_sees_one_difference(what, push):
    with pytest.raises(AssertionError, match=f"push {push}: {'reads' if what == 'extra' else what} differ"):
        wo.leaves_unchanged(Fake({what: push}), Fake(), PARTS, reads=(Fake.extra,), decode=True)
    with pytest.raises(AssertionError, match=f"push {push}"):
        wo.leaves_unchanged(Fake(), Fake({what: push}), PARTS, reads=(Fake.extra,), decode=True)


def test_leaves_unchanged_refuses_hops_that_are_all_zero():
    with pytest.raises(AssertionError, match="all zero"):
        wo.leaves_unchanged(Fake(silent=True), Fake(silent=True), PARTS)


class Drifts(Fake):
    """Its extra read differs in one byte at push 1 of the second run only."""

    def __init__(self):
        super().__init__()
        self.firsts = 0

    def push_wideband(self, slot, part, first=False):
        super().push_wideband(slot, part, first)
        self.firsts += first
        self.bend = {"extra": 1} if self.firsts == 2 else {}


def test_same_bytes_twice():
    again = wo.same_bytes_twice(Fake(), PARTS, Fake.extra)
    assert [int(p[1]) for p, _ in again] == [1, 2, 3]
    with pytest.raises(AssertionError, match="push 1: the second run"):
        wo.same_bytes_twice(Drifts(), PARTS, Fake.extra)
    with pytest.raises(AssertionError, match="push 0: all zero"):
        wo.same_bytes_twice(Fake(silent=True), PARTS, Fake.extra)
    with pytest.raises(AssertionError, match="all zero"):               # one member of the read is enough
        wo.same_bytes_twice(Fake(), PARTS, lambda d: (d.extra()[0], 0))


class Msk144Error(RuntimeError):
    def __init__(self, code):
        super().__init__(f"error {code}")
        self.code = code


class FakeHip:
    """hip.HipDecoder and hip.Msk144Error for the two refusal helpers; every handle made is kept."""

    Msk144Error = Msk144Error

    def __init__(self):
        self.made = []
        hip = self

        class HipDecoder(Fake):
            def __init__(self, channels, **cfg):
                super().__init__()
                assert channels == 1 and cfg == wo.wg.DECODE_CFG
                hip.made.append(self)

            def __enter__(self):
                return self

            def __exit__(self, *exc):
                self.close()

        self.HipDecoder = HipDecoder


def raises(code):
    def call(*_):
        raise Msk144Error(code)
    return call


def test_refuses_outside_wideband_mode():
    hip = FakeHip()
    wo.refuses_outside_wideband_mode(hip, [raises(wo.EINVAL), raises(wo.EINVAL)])
    for calls in ([raises(wo.EINVAL), lambda fresh: None], [raises(wo.ESTATE)], [raises(wo.EINVAL), raises(wo.ESTATE)]):
        with pytest.raises(FAILS):
            wo.refuses_outside_wideband_mode(hip, calls)
    assert len(hip.made) == 4 and all(d.closed for d in hip.made)      # a fresh handle each time, closed whatever happened


def test_unreadable():
    hip = FakeHip()
    wo.unreadable(hip, [raises(wo.ESTATE), raises(wo.ESTATE)])
    wo.unreadable(hip, [])
    for reads in ([raises(wo.ESTATE), lambda: None], [raises(wo.EINVAL)], [raises(wo.ESTATE), raises(wo.EINVAL)]):
        with pytest.raises(FAILS):
            wo.unreadable(hip, reads)


def test_code_of_and_the_shapes():
    assert wo.code_of(FakeHip(), raises(-7)) == -7
    assert (wo.OK, wo.EINVAL, wo.ESTATE) == (0, -1, -4)
    assert wo.SHAPE_NAMES[-2:] == ["one", "five"] and len(wo.SHAPE_NAMES) == 5
    assert len(wo.shape_of("one")["offsets"]) == 1 and wo.shape_of("rat") is wo.lc.SHAPES["rat"]
    hops = np.arange(12, dtype=np.int8).reshape(3, 2, 2)
    assert wo.Plain(hops).channels == 3 and np.array_equal(wo.Plain(hops).dump_wideband_hop(2), hops[2])


def test_handle_cache_closes_every_handle_also_when_the_body_raises():
    made = []

    def make(key):
        made.append((Fake(), Fake()) if key == "pair" else Fake())
        return made[-1]

    with wo.handle_cache(make) as get:
        assert get("pair") is get("pair") and get(3) is get(3) and get(3) is not get(4)
        assert len(made) == 3 and not made[1].closed
    assert all(d.closed for d in made[0]) and made[1].closed and made[2].closed
    del made[:]
    with pytest.raises(ZeroDivisionError):
        with wo.handle_cache(make) as get:
            get("pair"), get(1)
            1 / 0
    assert len(made) == 2 and all(d.closed for d in made[0]) and made[1].closed

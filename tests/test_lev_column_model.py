"""The Levenshtein column of `csrc/levcol.h`, modelled lane by lane (tests/lev_column_model.py), against plain dynamic
programming: both carry forms, several pair slots per 64-lane wave (a carry that leaks from a slot's last lane into the next
slot's first lane changes a distance), slots with idle lanes, random match masks in lanes outside their column range.  The
model asserts `vp & vn == 0` after every column of every lane.  No GPU needed."""
import numpy as np
import pytest

from lev_column_model import lev_dp, run_wave

ALPHABETS = (b"ab", b"acgt", bytes(range(97, 123)))
# (lanes per slot, pattern lengths to draw from): lengths around every 32-bit word boundary the slot can hold
SHAPES = [
    (1, [0, 1, 2, 31, 32]),
    (2, [0, 1, 31, 32, 33, 63, 64]),
    (3, [1, 32, 33, 63, 64, 65, 95, 96]),          # 21 slots, lane 63 idle
    (5, [7, 64, 96, 127, 128, 129, 159, 160]),     # 12 slots, lanes 60 .. 63 idle
    (16, [1, 33, 255, 256, 257, 480, 511, 512]),   # 4 x 16 lanes, no idle lane between slots
    (19, [40, 511, 512, 513, 575, 576, 577, 594, 607, 608]),   # 3 x 19 lanes
]


def _wave_cases():
    rng = np.random.default_rng(2024)
    cases = []
    for GL, mlens in SHAPES:
        P = 64 // GL
        # pairs per shape so that every shape contributes about the same number; 400+ pairs in all
        for _ in range(max(2, 70 // P)):
            alpha = ALPHABETS[rng.integers(0, 3)]
            pairs = []
            for g in range(P if rng.random() < 0.7 else rng.integers(1, P + 1)):
                m = int(mlens[rng.integers(0, len(mlens))])
                kind = rng.integers(0, 6)
                pat = bytes(rng.choice(list(alpha), m).tolist())
                if kind == 0:      # saturated horizontal deltas: nothing matches
                    pat, txt = b"a" * m, b"b" * m
                elif kind == 1:    # identical strings
                    txt = pat
                elif kind == 2:    # one symbol shorter / a few edits
                    t = bytearray(pat)
                    for _ in range(int(rng.integers(1, 6))):
                        if t and rng.random() < 0.5:
                            del t[int(rng.integers(0, len(t)))]
                        else:
                            t.insert(int(rng.integers(0, len(t) + 1)), int(alpha[rng.integers(0, len(alpha))]))
                    txt = bytes(t)
                elif kind == 3:    # empty text
                    txt = b""
                else:              # unrelated text of any length up to the pattern's slot and a little beyond
                    txt = bytes(rng.choice(list(alpha), int(rng.integers(0, min(32 * GL, 200) + 8))).tolist())
                pairs.append((pat, txt))
            cases.append((GL, pairs))
    return cases


CASES = _wave_cases()


def test_enough_cases():
    assert sum(len(p) for _, p in CASES) >= 400
    assert {GL for GL, _ in CASES} == {GL for GL, _ in SHAPES}


def test_lev_dp_known_answers():
    assert lev_dp(b"kitten", b"sitting") == 3
    assert lev_dp(b"", b"abc") == 3 and lev_dp(b"abc", b"") == 3 and lev_dp(b"", b"") == 0
    assert lev_dp(b"123456789", b"92346781") == 3
    assert lev_dp(b"a" * 40, b"b" * 33) == 40


@pytest.mark.parametrize("form", ["dpp", "mask"])
def test_column_model_matches_dp(form):
    rng = np.random.default_rng(7)
    for GL, pairs in CASES:
        want = [lev_dp(p, t) for p, t in pairs]
        assert run_wave(GL, pairs, form, rng) == want, (form, GL)


@pytest.mark.parametrize("form", ["dpp", "mask"])
def test_saturated_and_identical_slots_alternate(form):
    """64 one-lane slots, every lane a first lane: a saturated pair (every hp top bit set) beside an identical one (distance
    0) -- a carry that leaked across the slot boundary would change the 0."""
    pairs = [(b"a" * 32, b"b" * 32), (b"ab" * 16, b"ab" * 16), (b"a" * 32, b""), (b"a" * 31, b"a" * 31)] * 16
    assert run_wave(1, pairs, form, np.random.default_rng(0)) == [32, 0, 32, 0] * 16

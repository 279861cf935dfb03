"""Lane-by-lane model of the Levenshtein column of `csrc/levcol.h` (the recurrence of k_lev_f, k_lev_p2, k_lev_a2 and k_lev_ap),
in both carry forms, and a plain dynamic-programming reference.

A wave is 64 lanes; lane l belongs to pair slot l // GL and holds word w = l % GL of that slot's pattern (lanes past the last
whole slot form a partial slot that has no pair).  At iteration k lane w works on text column k - w.  `run_wave` walks the
iterations the way the kernels do and returns the distance of every slot's pair.

    "dpp"   the previous column's hp / hn words move down one lane (lane 0 gets 0) and take the per-lane constants
            hp_or / hn_and, which plant the first lane's carries (top DP row: hp = 1, hn = 0);
    "mask"  the carries are two 64-bit lane masks: (hp << 1) | carry is hp + hp + carry, whose carry-out -- hp's top bit --
            is collected from EVERY lane into a mask, shifted up one lane and patched with the mask of first lanes.

A lane outside its column range keeps vp / vn, is given a RANDOM match mask and passes its carries on like any other lane.
`vp & vn == 0` is asserted for every lane after every column.
"""
import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF


def lev_dp(a, b):
    """Plain row-by-row Levenshtein distance of two byte strings."""
    a = np.frombuffer(bytes(a), np.uint8)
    b = np.frombuffer(bytes(b), np.uint8)
    n = len(b)
    ramp = np.arange(n + 1)
    prev = ramp.copy()
    for i, ch in enumerate(a, 1):
        cur = np.empty(n + 1, np.int64)
        cur[0] = i
        cur[1:] = np.minimum(prev[:-1] + (b != ch), prev[1:] + 1)
        prev = np.minimum.accumulate(cur - ramp) + ramp   # cur[j] = min(cur[j], cur[j - 1] + 1), left to right
    return int(prev[n])


def _column(eq, c, hp_c, vp, vn):
    """One word-column given the two carry-ins as 0 / 1; returns (vp', vn', hp, hn)."""
    xv = eq | c | vn
    t = (c | eq) & vp
    sm = (t + vp) & M32
    d0 = (sm ^ vp) | xv
    hp = (vn | ~(d0 | vp)) & M32
    hn = d0 & vp
    hps = (hp + hp + hp_c) & M32
    hns = (hn + hn + c) & M32
    return (hns | ~(d0 | hps)) & M32, hps & d0, hp, hn


def run_wave(GL, pairs, form, rng):
    """pairs: (pattern, text) byte strings of the wave's slots in slot order, at most 64 // GL of them, patterns of at most
    32 * GL symbols.  Returns their distances."""
    assert form in ("dpp", "mask") and 1 <= GL <= 64 and len(pairs) <= 64 // GL
    lanes = range(64)
    w_of = [l % GL for l in lanes]
    slot_of = [l // GL for l in lanes]
    first = sum(1 << l for l in lanes if w_of[l] == 0)
    # match masks of every lane's pattern word
    pm = [dict() for _ in lanes]
    n_of = [0] * 64
    live = [False] * 64      # lane's slot has a pair with a non-empty pattern
    for g, (pat, txt) in enumerate(pairs):
        for l in range(g * GL, (g + 1) * GL):
            n_of[l] = len(txt)
            live[l] = len(pat) > 0
        for i, ch in enumerate(pat):
            d = pm[g * GL + i // 32]
            d[ch] = d.get(ch, 0) | (1 << (i % 32))
    vp = [M32] * 64
    vn = [0] * 64
    out_hp = [0] * 64
    out_hn = [0] * 64
    hp_in, hn_in = first, 0
    steps = max([len(t) + (len(p) + 31) // 32 - 1 for p, t in pairs if len(p) > 0] or [0])
    for k in range(steps):
        cop = con = 0
        new_hp, new_hn = [0] * 64, [0] * 64
        noise = rng.integers(0, 1 << 32, 64).tolist()
        for l in lanes:
            w = w_of[l]
            col = k - w
            valid = live[l] and 0 <= col < n_of[l]
            eq = pm[l].get(pairs[slot_of[l]][1][col], 0) if valid else noise[l]
            if form == "dpp":
                up_hp = (out_hp[l - 1] if l else 0) | (0x80000000 if w == 0 else 0)
                up_hn = (out_hn[l - 1] if l else 0) & (0 if w == 0 else M32)
                hp_c, c = up_hp >> 31, up_hn >> 31
            else:
                hp_c, c = (hp_in >> l) & 1, (hn_in >> l) & 1
            assert not (hp_c and c)
            nvp, nvn, hp, hn = _column(eq, c, hp_c, vp[l], vn[l])
            new_hp[l], new_hn[l] = hp, hn
            cop |= (hp >> 31) << l      # the carry-out of hp + hp + carry is hp's top bit, whatever the lane does next
            con |= (hn >> 31) << l
            if valid:
                vp[l], vn[l] = nvp, nvn
            assert vp[l] & vn[l] == 0
        out_hp, out_hn = new_hp, new_hn
        hp_in = ((cop << 1) | first) & M64
        hn_in = ((con << 1) & ~first) & M64
    res = []
    for g, (pat, txt) in enumerate(pairs):
        m, d = len(pat), len(txt)
        if m == 0:
            res.append(d)
            continue
        for w in range((m + 31) // 32):
            rows = M32 if w < (m + 31) // 32 - 1 else M32 >> (31 - ((m - 1) & 31))
            l = g * GL + w
            d += bin(vp[l] & rows).count("1") - bin(vn[l] & rows).count("1")
        res.append(d)
    return res

"""The pool planner of the loaders (annchor_amd/csrc/poollayout.h) on the host alone: tests/pool_layout_main.cpp is compiled
with the host compiler -- under AddressSanitizer and UBSan where an empty program builds and runs with them -- and fed every case
below on stdin.  The reference is the definition restated in NumPy: a member starts at the sum of the lengths before it, each
rounded up to the alignment."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "annchor_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover"]


def reference(lens, min_len, max_len, align, cap):
    lens = np.asarray(lens, dtype=np.int64)
    padded = (lens + align - 1) // align * align
    ends = np.cumsum(padded)
    short, long_, large = lens < min_len, lens > max_len, ends >= cap
    bad = np.flatnonzero(short | long_ | large)
    if bad.size:
        # the first member at fault; large counts the members before it, so a bad length in front of it is met first
        s = int(bad[0])
        return "refused %s %d" % ("short" if short[s] else "long" if long_[s] else "large", s)
    offs = ends - padded
    return " ".join(["ok", str(int(ends[-1])), str(int(lens.max()))] + [str(int(o)) for o in offs])


def cases():
    out = []
    for align in (1, 8, 16):
        big = 1 << 31
        out += [
            ([5, 3], 0, 100, align, big),                        # nx = 2
            ([0, 7, 9, 33], 0, 100, align, big),                 # an empty member first
            ([7, 9, 33, 0], 0, 100, align, big),                 # ... last
            ([0, 0, 0], 0, 100, align, big),                     # ... all of them
            ([1, 17, 40, 2, 16, 15], 0, 100, align, big),
            ([3, 100, 4], 0, 100, align, big),                   # a length equal to max_len
            ([3, 101, 4], 0, 100, align, big),                   # ... and one above it
            ([3, 4, -1, 5], 0, 100, align, big),                 # a negative length
            ([3, 4, -1, 5], 1, 100, align, big),
            ([3, 0, 5], 1, 100, align, big),                     # min_len = 1 with an empty member
            ([3, 1, 5], 1, 100, align, big),
            ([16, 32, 48, 16], 0, 100, align, big),              # lengths that are multiples of every alignment
            ([101, -1], 0, 100, align, big),                     # two faults: the first member's is reported
        ]
        lens = [20, 9, 30, 5]
        total = sum((l + align - 1) // align * align for l in lens)
        before_last = total - (lens[-1] + align - 1) // align * align
        out += [
            (lens, 0, 100, align, total),                        # the total reaches the cap exactly at the last member: refused there
            (lens, 0, 100, align, total + 1),                    # one element below the cap: taken
            (lens, 0, 100, align, before_last),                  # reached one member earlier
            (lens, 0, 100, align, before_last + 1),              # ... and passed by the last member only
        ]
    out.append(([2048] * 3, 0, 2048, 16, (1 << 31)))
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    d = tmp_path_factory.mktemp("pool_layout")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = SANITIZE
    r = subprocess.run([cxx] + flags + [str(probe), "-o", str(d / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(d / "probe")], capture_output=True).returncode != 0:
        flags = []   # no sanitizer runtime here: the outputs are still checked
    exe = d / "pool_layout_main"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + ["-I", CSRC, os.path.join(HERE, "pool_layout_main.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe), bool(flags)


def test_pool_layout_matches_numpy(program):
    exe, sanitized = program
    cs = cases()
    text = "".join("%d %d %d %d %d\n%s\n" % (len(l), lo, hi, al, cap, " ".join(map(str, l))) for l, lo, hi, al, cap in cs)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    assert len(got) == len(cs)
    for c, g in zip(cs, got):
        assert g == reference(*c), "case %r (sanitizers: %s)" % (c, sanitized)


def test_reference_sees_each_kind():
    """the cases exercise what they say: every kind of refusal and the accepted plans"""
    kinds = {reference(*c).split()[1] if reference(*c).startswith("refused") else "ok" for c in cases()}
    assert kinds == {"ok", "short", "long", "large"}

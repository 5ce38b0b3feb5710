"""Every exported call of match_calls.cpp and align_calls.cpp (the packed-text calls, the approximate matchers on both kinds of
text, the align calls, the IUPAC helpers), refused before the first HIP call: its return code and the text of smartgpu_last_error(),
compared with tests/golden/refusal_messages.json, which was recorded from the library as it stood before these calls left
api.cpp (`python tests/test_refusal_messages.py --record` with SMARTGPU_LIB naming that build).  A refactoring of the host
path may not change a code, a letter of a message or the order of two checks.

Without a device there is no text handle: every call passes NULL for it and, per case, ONE argument that a check reached
before the handle's refuses (or none: the handle's own refusal).  What the call may write — *count, the times, the output
arrays — holds sentinels before the call and must hold them after it."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))

from smart_amd import engine  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "refusal_messages.json")
XSIZE, GUARD64, GUARD8, CAP = 4200, 0xDEADBEEFDEADBEEF, 0xA5, 8

# name: (kind, longest m, largest k or None for a call without k, takes flags, reports distances)
MATCH = {}
for stem, max_m, max_k, flags in (("%s", XSIZE, None, False), ("%s_sets", XSIZE, None, False), ("%s_mis", XSIZE, 7, False),
                                  ("%s_sets_mis", XSIZE, 7, False), ("%s_edit", 64, 7, False), ("%s_sets_edit", 64, 7, False),
                                  ("%s_editl", 256, 31, True), ("%s_sets_editl", 256, 31, True)):
    MATCH["p" + stem % "search" + "64"] = ("count", max_m, max_k, flags, False)
    MATCH["p" + stem % "find" + "64"] = ("find", max_m, max_k, flags, max_k is not None)
for stem, max_m, max_k, flags in (("%s_edit", 64, 7, False), ("%s_edit_classes", 64, 7, False), ("%s_editl", 256, 31, True),
                                  ("%s_editl_classes", 256, 31, True), ("%s_mis", 64, 7, False), ("%s_mis_classes", 64, 7, False)):
    MATCH[stem % "search" + "64"] = ("count", max_m, max_k, flags, False)
    MATCH[stem % "find" + "64"] = ("find", max_m, max_k, flags, True)
for name in ("palign_edit64", "palign_sets_edit64", "align_edit64", "align_edit_classes64"):
    MATCH[name] = ("align", 64, 7, False, True)
for name in ("align_editl64", "align_editl_classes64"):
    MATCH[name] = ("align", 256, 31, False, True)
MATCH["psearch_batch64"] = ("batch_count", XSIZE, None, False, False)
MATCH["pfind_batch64"] = ("batch_find", XSIZE, None, False, False)


def match_cases():
    """(case id, call, the one argument that differs from a valid call)"""
    for name, (kind, max_m, max_k, flags, _) in MATCH.items():
        yield name + ":null_text", name, {}
        yield name + ":null_pattern", name, {"pat": "first is NULL" if kind.startswith("batch") else None}
        yield name + ":m_zero", name, {"m": 0}
        yield name + ":m_over", name, {"m": max_m + 1}
        if max_k is not None:
            yield name + ":k_over", name, {"k": max_k + 1}
        if flags:
            yield name + ":undefined_flag", name, {"flags": 2}
        if kind in ("count", "find"):
            yield name + ":null_count", name, {"count": None}
        if kind in ("find", "batch_find"):
            yield name + ":null_out_with_cap", name, {"out": None}
        if kind == "align":
            yield name + ":null_ends", name, {"ends": None}
            yield name + ":null_starts", name, {"out": None}
        if kind in ("batch_count", "batch_find"):
            yield name + ":K_zero", name, {"K": 0}
            yield name + ":null_P", name, {"pat": None}
            yield name + ":null_counts" if kind == "batch_count" else name + ":null_starts", name, {"starts": None}


class Sentinels:
    """What a call may write, and what it reads: the pattern (wide enough for 257 rows of classes), a set of two patterns"""

    def __init__(self):
        self.pat = np.full(300 * 32, 1, dtype=np.uint8)
        self.set = (ctypes.c_void_p * 2)(self.pat.ctypes.data, self.pat.ctypes.data)
        self.null_set = (ctypes.c_void_p * 2)(None, self.pat.ctypes.data)
        self.ends = np.arange(CAP, dtype=np.uint64)
        self.reset()

    def reset(self):
        self.count = ctypes.c_uint64(77)
        self.pre, self.run = ctypes.c_double(-1.0), ctypes.c_double(-2.0)
        self.out = np.full(CAP, GUARD64, dtype=np.uint64)
        self.starts = np.full(CAP, GUARD64, dtype=np.uint64)
        self.dist = np.full(CAP, GUARD8, dtype=np.uint8)
        self.ops = np.full(3 * CAP, GUARD64, dtype=np.uint64)
        self.small = np.full(16, GUARD8, dtype=np.uint8)
        self.planes = ctypes.c_int(-7)

    def untouched(self):
        return (self.count.value == 77 and self.pre.value == -1.0 and self.run.value == -2.0 and bool((self.out == GUARD64).all()) and
                bool((self.starts == GUARD64).all()) and bool((self.dist == GUARD8).all()) and bool((self.ops == GUARD64).all()) and
                bool((self.small == GUARD8).all()) and self.planes.value == -7 and bool((self.ends == np.arange(CAP)).all()))


def call_match(L, s, name, over):
    kind, _, max_k, flags, dist = MATCH[name]
    batch = kind.startswith("batch")
    a = dict(pat=ctypes.addressof(s.set) if batch else s.pat.ctypes.data, m=4, K=2, k=1, flags=0, count=ctypes.byref(s.count), out=s.out.ctypes.data,
             ends=s.ends.ctypes.data, starts=s.starts.ctypes.data)
    a.update(over)
    if a["pat"] == "first is NULL":
        a["pat"] = ctypes.addressof(s.null_set)
    args = [a["pat"], a["m"]] + ([a["K"]] if batch else []) + ([a["k"]] if max_k is not None else []) + ([a["flags"]] if flags else [])
    args += [None, 0, 100]  # the text handle, off, n
    if kind == "count":
        args += [a["count"], ctypes.byref(s.pre), ctypes.byref(s.run)]
    elif kind == "find":
        args += [a["out"]] + ([s.dist.ctypes.data] if dist else []) + [CAP, a["count"]]
    elif kind == "align":
        args += [a["ends"], CAP, a["out"], s.dist.ctypes.data, s.ops.ctypes.data]
    elif kind == "batch_count":
        args += [a["starts"], ctypes.byref(s.run)]
    else:
        args += [a["out"], CAP, a["starts"]]
    return getattr(L, "smartgpu_" + name)(*args)


# The calls around the matchers: (case id, call, arguments from the sentinels)
OTHER = [
    ("ptext_layout:no_values", "ptext_layout", lambda s: (100, 0, ctypes.byref(s.planes), ctypes.byref(s.count))),
    ("ptext_layout:five_values", "ptext_layout", lambda s: (100, 5, ctypes.byref(s.planes), ctypes.byref(s.count))),
    ("ptext_layout8:no_values", "ptext_layout8", lambda s: (100, 0, ctypes.byref(s.planes), ctypes.byref(s.count))),
    ("ptext_layout8:nine_values", "ptext_layout8", lambda s: (100, 9, ctypes.byref(s.planes), ctypes.byref(s.count))),
    ("ptext_pack:null_text", "ptext_pack", lambda s: (None,)),
    ("ptext_pack8:null_text", "ptext_pack8", lambda s: (None,)),
    ("ptext_upload:null_host", "ptext_upload", lambda s: (None, 4, 0)),
    ("ptext_upload8:null_host", "ptext_upload8", lambda s: (None, 4, 0)),
    ("ptext_free:null_text", "ptext_free", lambda s: (None,)),
    ("ptext_length:null_text", "ptext_length", lambda s: (None,)),
    ("ptext_device:null_text", "ptext_device", lambda s: (None,)),
    ("ptext_planes:null_text", "ptext_planes", lambda s: (None,)),
    ("ptext_bytes:null_text", "ptext_bytes", lambda s: (None,)),
    ("ptext_symbols:null_text", "ptext_symbols", lambda s: (None, s.small.ctypes.data)),
    ("ptext_symbols8:null_text", "ptext_symbols8", lambda s: (None, s.small.ctypes.data)),
    ("ptext_read:null_text", "ptext_read", lambda s: (None, 0, 4, s.small.ctypes.data)),
    ("ptext_probe_read_ms:null_text", "ptext_probe_read_ms", lambda s: (None, 1, ctypes.byref(s.pre))),
    ("iupac_sets:null_values", "iupac_sets", lambda s: (None, 4, b"ACGT", 4, s.small.ctypes.data)),
    ("iupac_sets:null_sets", "iupac_sets", lambda s: (b"ACGT", 4, b"ACGT", 4, None)),
    ("iupac_sets:no_values", "iupac_sets", lambda s: (b"ACGT", 0, b"ACGT", 4, s.small.ctypes.data)),
    ("iupac_sets:five_values", "iupac_sets", lambda s: (b"ACGNT", 5, b"ACGT", 4, s.small.ctypes.data)),
    ("iupac_sets:no_letter", "iupac_sets", lambda s: (b"ACGT", 4, b"ACJT", 4, s.small.ctypes.data)),
    ("iupac_sets8:null_values", "iupac_sets8", lambda s: (None, 4, b"ACGT", 4, s.small.ctypes.data)),
    ("iupac_sets8:nine_values", "iupac_sets8", lambda s: (b"-ACGNTXYZ", 9, b"ACGT", 4, s.small.ctypes.data)),
    ("iupac_sets8:no_letter", "iupac_sets8", lambda s: (b"ACGNT", 5, b"AC!T", 4, s.small.ctypes.data)),
    ("iupac_revcomp:null_out", "iupac_revcomp", lambda s: (b"ACGT", 4, None)),
    ("iupac_revcomp:no_letter", "iupac_revcomp", lambda s: (b"ACJT", 4, s.small.ctypes.data)),
]

CASES = [(cid, name, over) for cid, name, over in match_cases()] + [(cid, name, args) for cid, name, args in OTHER]


def answer(L, s, name, how):
    """{"rc", "error"} of one case.  A call that sets no message leaves the one of the refusal made just before it."""
    s.reset()
    assert L.smartgpu_iupac_revcomp(None, 1, None) == -3  # a known message to start from
    rc = call_match(L, s, name, how) if isinstance(how, dict) else getattr(L, "smartgpu_" + name)(*how(s))
    return {"rc": rc, "error": L.smartgpu_last_error().decode()}


@pytest.fixture(scope="module")
def library():
    engine.build()
    return engine.lib()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_names_exactly_these_cases(golden):
    assert sorted(golden) == sorted(c[0] for c in CASES) and len(golden) == len(CASES)


def test_every_moved_call_is_covered():
    """every function the two units define with C linkage has at least one case"""
    import re
    csrc = os.path.join(os.path.dirname(HERE), "smart_amd", "csrc")
    src = open(os.path.join(csrc, "match_calls.cpp")).read() + open(os.path.join(csrc, "align_calls.cpp")).read()
    defined = set(re.findall(r"^(?:int|void|uint64_t|smartgpu_ptext\*) smartgpu_([a-z0-9_]+)\(", src, flags=re.M))
    assert len(defined) >= 50, sorted(defined)
    assert defined == {name for _, name, _ in CASES}, defined ^ {name for _, name, _ in CASES}


@pytest.mark.parametrize("cid,name,how", CASES, ids=[c[0] for c in CASES])
def test_refusal_is_as_recorded(library, golden, cid, name, how):
    s = Sentinels()
    got = answer(library, s, name, how)
    assert got == golden[cid], (cid, got, golden[cid])
    assert s.untouched(), cid


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: SMARTGPU_LIB=<library> python tests/test_refusal_messages.py --record")
    lib, sent = engine.lib(), Sentinels()
    recorded = {}
    for cid, name, how in CASES:
        recorded[cid] = answer(lib, sent, name, how)
        assert sent.untouched(), cid
    with open(GOLDEN, "w") as f:
        json.dump(recorded, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases from %s" % (len(recorded), engine.LIB_PATH))

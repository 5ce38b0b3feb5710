"""The C ABI's call layer on the CPU: match_calls.cpp and align_calls.cpp, the real units, linked against the stubs of
tests/host_calls_check.cpp (what api.cpp, k_planes.hip and the self-registering kernel units give them in the library), with
text handles the driver fills in itself.  Compiled with AddressSanitizer and UBSan, run as a program without a preload.

So everything a call decides before it needs a device RUNS here: the order of its checks (every pair of two violations
answers as the earlier one alone), that a refused call writes nothing and asks for no device, the refusal of a kernel that is
not linked, what is answered without a launch, and the messages that need a live handle.  The driver asserts the
invariants; this test compares its lines with tests/golden/host_call_cases.json, recorded from the library as it stood
before the align calls got one path (`python tests/test_host_calls.py --record`), and ties that fixture to
tests/golden/refusal_messages.json, which was recorded through the library itself."""
import functools
import json
import os
import subprocess
import sys
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "smart_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden", "host_call_cases.json")
REFUSALS = os.path.join(HERE, "golden", "refusal_messages.json")
UNITS = ("match_calls.cpp", "align_calls.cpp")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-result", "-Wno-unused-value", "-Wno-unused-function"] + SANITIZE
FIELDS = ("rc", "device", "launchers", "written", "error")


def run_driver(workdir, units=UNITS):
    """{case id: {rc, device, launchers, written, error}} as the driver prints them, in its order"""
    sources = {"driver": os.path.join(HERE, "host_calls_check.cpp")}
    sources.update({u: os.path.join(CSRC, u) for u in units})
    procs = [(u, subprocess.Popen([HIPCC] + FLAGS + ["--offload-arch=gfx950", "-c", "-o", os.path.join(workdir, u + ".o"), src],
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)) for u, src in sources.items()]
    for u, p in procs:
        out, _ = p.communicate(timeout=900)
        assert p.returncode == 0, (u, out[-4000:])
    exe = os.path.join(workdir, "host_calls_check")
    subprocess.check_call([HIPCC, "-o", exe] + SANITIZE + [os.path.join(workdir, u + ".o") for u in sources])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr.strip() == "0 failures", r.stderr[-4000:]
    cases = {}
    for line in r.stdout.splitlines():
        cid, rc, dev, launch, written, error = line.split("\t", 5)
        assert cid not in cases, cid
        cases[cid] = dict(zip(FIELDS, (None if rc == "None" else int(rc), int(dev), int(launch), written, error)))
    return cases


@functools.lru_cache(maxsize=None)
def driver_cases():
    """run_driver once per session: tests/test_text_mis.py reads the same cases"""
    with tempfile.TemporaryDirectory() as work:
        return run_driver(work)


@pytest.fixture(scope="module")
def cases():
    return driver_cases()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def condensed(cases):
    """What the fixture holds of the driver's cases, one line each: [rc, device, launchers, written, error], and for a single
    violation (order/<call>/<form>) a sixth entry, the number of its pairs order/<call>/<form>+<later form>.  A pair has no
    line of its own: its line IS the earlier violation's, which test_every_case_is_as_recorded asserts field by field.  The
    null/ cases have none either: tests/golden/refusal_messages.json holds their codes and messages."""
    out = {}
    for cid, v in cases.items():
        if cid.startswith("null/"):
            continue
        if cid.startswith("order/") and "+" in cid:
            out[cid.split("+")[0]][5] += 1
        else:
            out[cid] = [v[f] for f in FIELDS] + ([0] if cid.startswith("order/") else [])
    return out


def test_every_case_is_as_recorded(cases, golden):
    got = condensed(cases)
    assert list(got) == list(golden)
    differing = {cid: (got[cid], golden[cid]) for cid in got if got[cid] != golden[cid]}
    assert not differing, list(differing.items())[:5]
    pairs = [cid for cid in cases if cid.startswith("order/") and "+" in cid]
    for cid in pairs:  # every field of a pair is the recorded line of its earlier violation
        assert [cases[cid][f] for f in FIELDS] == golden[cid.split("+")[0]][:5], (cid, cases[cid])
    assert len(pairs) == sum(v[5] for cid, v in golden.items() if cid.startswith("order/")) > 1500 and len(golden) > 500


def test_the_fixture_agrees_with_the_one_recorded_through_the_library(cases):
    """every case of refusal_messages.json that needs no call behind the device's context: the same code and message"""
    with open(REFUSALS) as f:
        refusals = json.load(f)
    beyond = {"ptext_upload:null_host", "ptext_upload8:null_host"}  # smartgpu_text_upload is api.cpp's: a stub here
    assert beyond < set(refusals)
    for cid, want in refusals.items():
        if cid not in beyond:
            got = cases["null/" + cid]
            assert (got["rc"], got["error"]) == (want["rc"], want["error"]), (cid, got, want)
            assert got["device"] == 0 and got["written"] == "-", (cid, got)
    assert {c[5:] for c in cases if c.startswith("null/")} == set(refusals) - beyond


def test_checks_come_before_the_missing_kernel_and_that_before_the_device(cases):
    device = {c: v for c, v in cases.items() if c.startswith("device/")}
    missing = {c: v for c, v in cases.items() if c.startswith("missing/")}
    assert len(device) >= 36 and len(missing) >= 36
    for cid, v in device.items():
        assert (v["rc"] in (-4, None), v["device"], v["launchers"], v["written"]) == (True, 1, 0, "-") and "(stub) device_ctx_flushed" in v["error"], (cid, v)
    part_of_every_program = {"psearch64", "pfind64", "psearch_batch64", "pfind_batch64", "psearch_sets64", "pfind_sets64", "psearch_mis64", "pfind_mis64",
                             "psearch_sets_mis64", "pfind_sets_mis64", "ptext_pack8:four_values"}
    for cid, v in missing.items():
        if cid[len("missing/"):] in part_of_every_program:  # the two-plane kinds of k_planes.hip: no such refusal
            assert v["device"] == 1 and "(stub) device_ctx_flushed" in v["error"], (cid, v)
        else:
            assert v["device"] == 0 and v["launchers"] == 0 and v["written"] == "-", (cid, v)
            assert "this program holds no " in v["error"] and v["error"].endswith(".hip is not linked)"), (cid, v)
    for cid, v in cases.items():
        if cid.startswith(("order/", "null/", "answer/")):
            assert v["device"] == 0 and v["launchers"] == 0, (cid, v)
        if cid.startswith("order/"):
            assert v["rc"] == -3 and v["written"] == "-", (cid, v)


def test_answers_without_a_launch(cases):
    for call in ("psearch_sets64", "pfind_sets64"):
        assert cases["answer/%s/full_sets" % call]["rc"] == 0
    assert cases["answer/psearch_sets64/full_sets"]["written"] == "count=47 times=0,0"
    assert cases["answer/pfind_sets64/full_sets"]["written"] == "count=47 out=47 from 10 by one"
    short = cases["answer/pfind_sets64/full_sets_cap_one_short"]
    assert (short["rc"], short["written"], short["error"]) == (-5, "count=47", "pfind_sets64: 47 occurrences, room for 46")
    assert cases["answer/align_editl64/no_ends"] == dict(zip(FIELDS, (0, 0, 0, "-", "(no message)")))
    assert cases["answer/find_edit64/n_plus_k_below_m"]["written"] == "count=0" and cases["answer/find_mis64/m_above_n"]["written"] == "count=0"
    assert cases["answer/pfind64/foreign_bytes"]["written"] == "count=0"


def test_messages_that_need_a_live_handle(cases):
    assert cases["order/pfind_sets_mis64/set_code"]["error"] == "set pattern: position 2: set 0x11 names a code >= 4, the number of values the text holds"
    assert cases["order/align_editl64/end_outside"]["error"] == "align_editl64: ends[1] = 90 outside the range [10,+80)"
    assert cases["order/palign_edit64/three_planes"]["error"].startswith("palign_edit64: three-plane texts (five to eight values) are not offered here")
    assert cases["order/psearch_batch64/batch_of_7885_on_three_planes"]["error"].startswith("psearch_batch: 7885 patterns on a three-plane text, at most 7884 per call")
    assert cases["handle/ptext_symbols@three_planes"]["error"].startswith("ptext_symbols: a three-plane text holds 6 values")
    assert cases["order/find_editl64/off_wraps"]["error"] == "find_editl64: range [18446744073709551615,+2) outside the text (100 bytes)"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_host_calls.py --record")
    with tempfile.TemporaryDirectory() as work:
        recorded = run_driver(work)
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(cid) + ":" + json.dumps(v, separators=(",", ":")) for cid, v in condensed(recorded).items()) + "\n}\n")
    print("recorded %d cases" % len(recorded))

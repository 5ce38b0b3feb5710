"""What the packed-text calls decide on the host (smart_amd/csrc/planes_host.hpp), on the CPU: tests/packed_host_check.cpp
checks every bit of the planes that encode_pattern and encode_sets write against the definition in planes.hpp — text
alphabets of 1 to 4 values, m = 1, 31, 32, 33, 64, 65 and SMARTGPU_XSIZE, patterns with no, one and several foreign bytes,
sets with empty, full and singleton positions, zero bits from m up to the planes' end — with the foreign and empty counts,
the full flag and the first position of a bad set; and order_spans on its table and its sort path, with shift 0 and
kMisShift, over ranges whose s_begin is no multiple of 128: ascending input, shuffled spans, a span in two pieces, a key
outside the range, a descending and an equal pair inside a span; order_editl on sorted, shuffled and no entries, and its
four refusals (an end position twice, one below lo, one above hi, a distance of k + 1); and find_outcome — which of "cursor
beyond the bound", "list complete", "more than cap", "fits cap but the device had no room" a find's cursor means — for
bound 1 and 5, cap 0, 1, bound - 1, bound, bound + 1, room_got 0 and min(cap, bound), every total from 0 to bound + 1, against
a table written out by hand.
The program is compiled with AddressSanitizer and UBSan: a write past a plane or a read past the entries ends it."""
import os
import re
import subprocess

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"


def test_encoders_and_order_spans_on_the_host(tmp_path):
    exe = tmp_path / "packed_host_check"
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "packed_host_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # encode_pattern: 4 alphabets x 7 lengths x 3 kinds of pattern x with and without SKIP; encode_sets: 4 x 7 x 2 rules for
    # empty positions x (3 kinds of sets + 1 bad set); order_spans: 2 shifts x 2 ranges x (9 on the table path + 7 on the sort path);
    # find_outcome: 5 caps x 2 room_got x (bound + 2 totals) for bound 1 and 5; order_editl: 3 accepted + 4 refused
    want = 4 * 7 * 3 * 2 + 4 * 7 * 2 * 4 + 2 * 2 * (9 + 7) + 5 * 2 * (3 + 7) + 3 + 4
    assert r.returncode == 0 and failures == 0 and cases == want, r.stdout[-4000:] + r.stderr[-2000:]

"""Differential fuzz of the approximate matchers on packed texts under -m gpu: planes_sets_*, planes_mis_*, planes_sets_mis_*,
planes_edit_*, planes_editl_* and planes_edit_align on the cases tests/packed_fuzz.py draws under its committed seed — value
sets, lengths around the kernels' runs, skewed, periodic, run-heavy, one-value and segmented texts with a field of
near-copies next to noise, every k, the edges of every column width, byte and set patterns, a sub-range that starts and ends
mid-dword — one grid sweep each; later trips and positions past 2^32 stay with tests/test_packed_at_size_gpu.py.

Per case and range: the count call and the find call against the family's by-definition reference (exact equality of count,
positions or ends, and distances), a find with cap one short of the count, cap = 0 with NULL buffers, and the identities
include/smartgpu.h promises, which cost no reference run (mis at k = 0 is pfind, sets_mis at k = 0 is sets, singleton sets give
the byte call's answers and the other way round, edit at k = 0 is pfind + m - 1, editl with and without all_blocks, editl at
m <= 64 and k <= 7 is edit); for align the find's ends, a shuffled subset with duplicates and random ends of the range, each
with and without operations, against align_many, every returned alignment replayed.  Every message carries (family, index)
and the drawn shape: tools/packed_fuzz_gpu.py --family F --start I --cases 1 runs that case alone.

Each test ends with the strata its run must have met (packed_fuzz.missing_strata); tests/test_packed_fuzz.py asserts the same
from the generator and the references alone, so a failure of the closing assertion here has its reason on the GPU side.

The committed run (packed_fuzz.SEED, packed_fuzz.CASES), as measured on an MI355X machine — nearly all of the time is the CPU
reference — cases / comparisons / seconds per test: sets 256 / 2,169 / 0.6, mis 256 / 3,922 / 0.8, sets_mis 256 / 3,209 / 0.7,
edit 256 / 3,205 / 0.8, editl 128 / 2,590 / 3.2, align 96 / 2,337 / 2.1; 8.4 s for the module.  The floor of the counts
is the strata below; they are set so that no test takes more than a few seconds.  The mutants the module was tried against:
profiles/packed/RESULTS.md, "Differential fuzz".  No wrong answer found; product code unchanged."""
import time

import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402

import packed_fuzz as pf  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


@pytest.mark.parametrize("family", pf.FAMILIES)
def test_differential_fuzz(family):
    tally = pf.Tally()
    t0 = time.time()
    for index in range(pf.CASES[family]):
        pf.check(pf.draw(family, index), tally)
    print("packed fuzz %s: %d cases, %d comparisons in %.1f s" % (family, len(tally.cases), tally.comparisons, time.time() - t0))
    assert len(tally.cases) == pf.CASES[family]
    assert pf.missing_strata(family, tally.cases, tally.shapes) == []

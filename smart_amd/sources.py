"""Which source files decide the code of which kernel (smart_amd/csrc: one translation unit — one code object —
per kernel family), and a sha256 over such a set.  Measurements that are only valid for the kernel source they were
taken on (profiles/pmc_traffic.json: roofline.traffic of bench.py) are bound to the FAMILY's sha, so an edit to
bm_scan does not void the PMC traffic of so_runs."""
import hashlib
import os

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
# every kernel unit includes these (device helpers, argument structs, launch geometry)
COMMON = ("dev_common.hpp", "kernels.hpp", "launch_common.hpp")
UNITS = {
    "k_hor": ("k_hor.hip",),
    "k_horm": ("k_horm.hip", "multi.hpp"),
    "k_hormf": ("k_hormf.hip", "multi_find.hpp", "multi.hpp"),
    "k_hors": ("k_hors.hip", "sample.hpp", "multi.hpp"),
    "k_horg": ("k_horg.hip", "gram_skip.hpp"),
    "k_bmg": ("k_bmg.hip", "gram_skip.hpp"),
    "k_bm": ("k_bm.hip",),
    "k_bndm": ("k_bndm.hip",),
    "k_bndmx": ("k_bndmx.hip",),
    "k_so": ("k_so.hip", "runs_common.hpp"),
    "k_kmp": ("k_kmp.hip", "runs_common.hpp"),
    "k_packed": ("k_packed.hip",),
    "k_util": ("k_util.hip", "text_rate.hpp"),
    "k_planes": ("k_planes.hip", "planes.hpp"),
    "k_planes3": ("k_planes3.hip", "planes3.hpp", "planes3_host.hpp", "planes.hpp"),
    "k_pedit": ("k_pedit.hip", "pedit.hpp", "pedit_host.hpp", "edit_step.hpp", "planes.hpp"),
    "k_peditl": ("k_peditl.hip", "peditl.hpp", "peditl_host.hpp", "edit_block.hpp", "planes.hpp"),
    "k_palign": ("k_palign.hip", "palign.hpp", "edit_align.hpp", "pedit.hpp", "pedit_host.hpp", "edit_step.hpp", "planes.hpp"),
    "k_tedit": ("k_tedit.hip", "text_tile.hpp", "tedit.hpp", "tedit_host.hpp", "edit_step.hpp", "planes.hpp"),
    "k_teditl": ("k_teditl.hip", "teditl.hpp", "teditl_host.hpp", "edit_block.hpp", "planes.hpp"),
    "k_tmis": ("k_tmis.hip", "text_tile.hpp", "tmis.hpp", "tmis_host.hpp", "tedit_host.hpp", "edit_step.hpp", "planes.hpp"),
    "k_talignl": ("k_talignl.hip", "talignl.hpp", "alignl_band.hpp", "talign_host.hpp", "tedit_host.hpp", "teditl_host.hpp", "edit_align.hpp", "edit_block.hpp", "edit_step.hpp", "planes.hpp"),
    "k_palignl": ("k_palignl.hip", "palignl.hpp", "alignl_band.hpp", "talign_host.hpp", "tedit_host.hpp", "peditl_host.hpp", "edit_align.hpp", "edit_block.hpp", "edit_step.hpp", "planes.hpp"),
    "k_talign": ("k_talign.hip", "talign.hpp", "talign_host.hpp", "tedit.hpp", "tedit_host.hpp", "edit_align.hpp", "edit_step.hpp", "planes.hpp"),
}
KERNEL_UNIT = {
    "hor_scan": "k_hor", "hor_multi_scan": "k_horm", "hor_multi_find": "k_hormf", "hor_sample_scan": "k_hors", "text_sample_build": "k_hors","hor_scan_bp": "k_hor", "hor_scan_gram": "k_horg", "bm_scan_gram": "k_bmg", "bm_scan": "k_bm", "bndm_scan": "k_bndm", "sbndm_scan": "k_bndmx",
    "bndml_scan": "k_bndmx", "so_runs": "k_so", "kmp_runs": "k_kmp", "packed_scan": "k_packed", "packed_find": "k_packed",
    "generate_text": "k_util", "tile_fill": "k_util", "text_alphabet": "k_util", "text_histogram": "k_util", "probe_read": "k_util",
    "planes_pack": "k_planes", "planes_scan": "k_planes", "planes_find": "k_planes",
    "planes_sets_scan": "k_planes", "planes_sets_find": "k_planes",
    "planes_mis_scan": "k_planes", "planes_mis_find": "k_planes",
    "planes_sets_mis_scan": "k_planes", "planes_sets_mis_find": "k_planes",
    "planes3_pack": "k_planes3", "planes3_scan": "k_planes3", "planes3_find": "k_planes3",
    "planes_edit_scan": "k_pedit", "planes_edit_find": "k_pedit",
    "planes_editl_scan": "k_peditl", "planes_editl_find": "k_peditl",
    "planes_edit_align": "k_palign",
    "text_edit_scan": "k_tedit", "text_edit_find": "k_tedit",
    "text_editl_scan": "k_teditl", "text_editl_find": "k_teditl",
    "text_edit_align": "k_talign",
    "text_editl_align": "k_talignl",
    "planes_editl_align": "k_palignl",
    "text_mis_scan": "k_tmis", "text_mis_find": "k_tmis",
}


def unit_files(unit):
    return [os.path.join(CSRC, f) for f in UNITS[unit] + COMMON]


def unit_sha256(unit, read=None):
    """sha256 over the unit's own sources and the common headers, in a fixed order.  `read(path) -> bytes`
    replaces the file system (tools/collect_profiles.py hashes the COMMITTED sources through git show)."""
    h = hashlib.sha256()
    for p in unit_files(unit):
        data = read(p) if read else open(p, "rb").read()
        h.update(os.path.basename(p).encode() + b"\0" + data + b"\0")
    return h.hexdigest()


def kernel_sha256(kernel, read=None):
    return unit_sha256(KERNEL_UNIT[kernel], read)


def all_unit_shas(read=None):
    return {u: unit_sha256(u, read) for u in UNITS}

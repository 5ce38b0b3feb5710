"""smart_amd — MI355X-native exact string matching behind SMART's `search()` plugin surface.

The product is the C-ABI shared library `smart_amd/csrc/libsmartgpu.so`
(include/smartgpu.h); this package is the thin ctypes binding plus a Python
mirror of SMART's harness vocabulary (texts, patterns, algorithms).
"""
from .engine import (ALGOS, MIN_M, MultiText, PackedText, Plan, SmartGpuError, Text, algo_id, build_table, device_count, kernel_for,  # noqa: F401
                     edit_cigar, find, find_batch, find_batch_max, find_width, iupac_revcomp, iupac_sets, lib, palign_edit, palign_sets_edit, pfind, pfind_batch, pfind_edit, pfind_edit_align, pfind_mis, pfind_sets, pfind_sets_edit,
                     pfind_editl, pfind_sets_editl, psearch_editl, psearch_sets_editl,
                     palign_editl, palign_sets_editl, pfind_editl_align, pfind_sets_editl_align,
                     pfind_sets_mis, psearch, psearch_batch, psearch_edit, psearch_mis, psearch_sets, psearch_sets_edit, psearch_sets_mis,
                     ptext_layout, ptext_layout8, search,
                     align_edit, align_edit_classes, find_edit_align, find_edit_classes_align,
                     align_editl, align_editl_classes, find_editl_align, find_editl_classes_align,
                     byte_classes, find_edit, find_edit_classes, search_edit, search_edit_classes,
                     find_editl, find_editl_classes, search_editl, search_editl_classes,
                     find_mis, find_mis_classes, search_mis, search_mis_classes, search_batch, search_host, version)

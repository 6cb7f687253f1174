"""sx_result_fold_device, what the compiler made of stringsext_amd/csrc/sx_fold_dev.hip (no GPU needed): the per-kernel resource
remarks the Makefile keeps next to the object.  The file also instantiates rocprim's scan; its kernels are not ours and are not
judged here."""
import os
import re

from test_kernel_resources import CSRC, remarks

KERNELS = ["fold_measure_kernel", "fold_place_kernel"]


def constant(path, name):
    with open(os.path.join(CSRC, path)) as f:
        found = re.findall(r"\b%s\s*=\s*(\d+)u?\s*[;,]" % name, f.read())
    assert len(found) == 1, (path, name, found)
    return int(found[0])


def test_the_fold_kernels_have_no_scratch_no_spills_the_table_in_lds_and_three_workgroups_per_cu():
    rows = {k: v for k, v in remarks("sx_fold_dev").items() if not k.startswith("rocprim::")}
    assert sorted(rows) == KERNELS, sorted(rows)
    lds, table = constant("sx_fold_dev.hip", "kFoldLdsBytes"), constant("sx_fold_table.inc", "kFoldTableBytes")
    groups, waves = constant("sx_rows_dev.hpp", "kRowsGroupsPerCu"), constant("sx_rows_dev.hpp", "kRowsWaves")
    assert table <= lds < table + 16 and lds <= 20 * 1024                # the table, next to nothing else
    for k, v in rows.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0 and v["Dynamic Stack"] == "False", (k, v)
        assert v["LDS Size [bytes/block]"] == lds, (k, v)                # what the source states: no array of a lane's went there
        assert groups * v["LDS Size [bytes/block]"] <= 160 * 1024, (k, v)      # a CU of gfx950 has 160 KiB
        # the grid: kRowsGroupsPerCu workgroups of kRowsWaves wavefronts per CU, over 4 SIMDs — resident together only if the
        # registers allow as many; R of tests/test_gpu_fold_device.py rests on the same numbers
        assert v["Occupancy [waves/SIMD]"] * 4 >= groups * waves, (k, v)

"""The step kernels' register budget, read from the built library's code-object metadata (tools/kernel_resources.py; no GPU): the lean job-queue kernel keeps
its 168 VGPRs (three waves per SIMD), no step kernel needs more VGPRs, VGPR spills or scratch than the parent commit's build recorded in
profiles/sgpr_diet/kernels_parent.md, and the scalar-register spills of the metric's kernel stay below the parent's."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

METRIC = "void kp::kp_step_queue_kernel<false, true>(kp::StepArgs)"


def _parent_name(name):
    """the parent's kernel a step kernel of this build is held to: the profiler became a third template argument of kp_step_kernel / kp_step_kernel_xc, and the
    parent ran the one instantiation <NT, OBJ> with and without profiling"""
    return re.sub(r"(kp_step_kernel(?:_xc)?<\d+, (?:true|false)), (?:true|false)>", r"\1>", name)


@pytest.fixture(scope="module")
def tables():
    import kernel_resources
    from kinpoly_amd import build as kpbuild
    this = {k: v for k, v in kernel_resources.table(kpbuild.build_native()).items() if "kp_step_" in k}
    parent = kernel_resources.parse(open(os.path.join(ROOT, "profiles", "sgpr_diet", "kernels_parent.md")).read())
    return this, {k: v for k, v in parent.items() if "kp_step_" in k}


def test_the_tables_cover_the_same_step_kernels(tables):
    this, parent = tables
    assert len(parent) == 14 and METRIC in parent and METRIC in this
    assert {_parent_name(k) for k in this} == set(parent)
    # the product instantiations plus one profiling instantiation per one-workgroup-per-env kernel
    assert len(this) == len(parent) + sum("kp_step_kernel" in k for k in parent)


def test_lean_queue_kernel_keeps_three_waves_per_simd(tables):
    this, _ = tables
    assert this[METRIC]["vgpr"] <= 168 and this[METRIC]["agpr"] == 0


def test_no_step_kernel_needs_more_registers_or_scratch_than_the_parent(tables):
    this, parent = tables
    worse = [(k, c, v[c], parent[_parent_name(k)][c]) for k, v in sorted(this.items()) for c in ("vgpr", "vgpr_spill", "scratch_bytes", "lds_bytes")
             if v[c] > parent[_parent_name(k)][c]]
    assert not worse, worse


def test_scalar_register_spills_of_the_metric_kernel_are_below_the_parent(tables):
    this, parent = tables
    print({k: (parent[_parent_name(k)]["sgpr_spill"], v["sgpr_spill"]) for k, v in sorted(this.items())})
    assert this[METRIC]["sgpr_spill"] < parent[METRIC]["sgpr_spill"]

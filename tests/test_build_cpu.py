"""CPU tests of build.py's variant mode, without compiling: a variant unit's command line is the product's plus the extra flags, an unknown
unit is refused, and a variant library links the product's objects except the units it recompiles."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("ts2d_build_variants", os.path.join(ROOT, "triangle-splatting_amd", "build.py"))
build = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(build)

EXTRA = ["-DTSG_FWD_WAVES=6", "-mllvm", "-amdgpu-sched-strategy=max-ilp"]


@pytest.mark.parametrize("unit, key", [("render_group_fwd", "render_group.hip@fwd"), ("aux_losses", "aux_losses.hip"), ("api", "api.hip")])
def test_variant_command_is_the_product_command_plus_the_extra_flags(unit, key):
    product = build.command(unit, cc="hipcc")
    src = os.path.join(build.CSRC, key.partition("@")[0])
    assert product == ["hipcc", *build.COMMON, *build.SOURCES[key], "-c", src, "-o", os.path.join(build.OBJ_DIR, unit + ".o")]
    variant = build.command(unit, EXTRA, variant="x", cc="hipcc")
    assert variant == product[:-4] + EXTRA + ["-c", src, "-o", os.path.join(build.VARIANT_DIR, "x", unit + ".o")]


def test_lab_units_keep_their_own_flags():
    variant = build.command("lab/api", ["-DTS2D_STATS"], variant="x", cc="hipcc")
    assert variant[:-4] == ["hipcc", *build.COMMON, *build.LAB_SOURCES["api.hip"], "-DTS2D_STATS"]
    assert variant[-1] == os.path.join(build.VARIANT_DIR, "x", "lab", "api.o")


def test_unknown_units_are_refused():
    with pytest.raises(ValueError, match="unknown unit"):
        build.command("render_group", EXTRA, variant="x", cc="hipcc")  # two units since the forward / backward split: no such object
    with pytest.raises(ValueError, match="unknown unit"):
        build.build(variant="x", extra={"render_group.hip": EXTRA})
    with pytest.raises(ValueError, match="unknown unit"):
        build.build(variant="x", extra={"lab/api": ["-DTS2D_STATS"]})  # a lab unit without lab=True


@pytest.mark.parametrize("lab", [False, True])
def test_variant_objects_replace_exactly_the_named_units(lab):
    extra = {"render_group_bwd": ["-DTS2D_STATS"], "depth_order": EXTRA}
    if lab:
        extra["lab/lab_hooks"] = ["-DNDEBUG"]
    product, variant = build.objects(lab), build.objects(lab, "x", extra)
    assert len(variant) == len(product) == len(build.units(lab))
    for unit, p, v in zip(build.units(lab), product, variant):
        assert p == os.path.join(build.OBJ_DIR, unit + ".o")
        assert v == (os.path.join(build.VARIANT_DIR, "x", unit + ".o") if unit in extra else p)

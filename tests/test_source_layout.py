"""One translation unit per concern (source layout): what each object of libumpc_mi355x.so was compiled from is what
the compiler recorded in its depfile, and build() rebuilds from exactly that. CPU only: the build needs no GPU."""
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# generated code: the step path alone may read it
GENERATED = ("umpc_gen.h", "umpc_admm_asm", "umpc_step_asm", "umpc_quad64_tab.h", "umpc_n3_general.h")


def _deps(lib, unit):
    """the files the depfile of csrc/<unit> names, as the compiler wrote them (relative to csrc)"""
    txt = open(os.path.join(lib.OBJ_DIR, unit + ".o.d")).read().replace("\\\n", " ")
    return txt.split(": ", 1)[1].split()


def test_units_depend_on_what_the_compiler_read():
    from robobee3d_amd import _lib
    _lib.build()
    for unit in ("umpc_scoring.hip", "umpc_sim.hip"):
        deps = _deps(_lib, unit)
        assert unit in deps and "umpc_handle.h" in deps, (unit, deps)
        assert not [d for d in deps if os.path.basename(d).startswith(GENERATED)], (unit, deps)
        assert "umpc_step.h" not in deps, (unit, deps)
        assert not [d for d in deps if os.path.isabs(d)], (unit, deps)      # local files only: the same on every machine
    step = _deps(_lib, "umpc_mi355x.hip")
    assert "umpc_step_asm.h" in step and "umpc_step.h" in step and "umpc_handle.h" in step, step
    assert not [d for d in step if os.path.basename(d) in ("umpc_score.h", "umpc_models.h")], step
    # every hand-written unit has an object, a depfile and a resource record, and build() knows it
    units = sorted(glob.glob(os.path.join(_lib.CSRC, "*.hip")))
    assert units == sorted(_lib.UNITS) and len(units) == 4
    for src in units:
        obj = os.path.join(_lib.OBJ_DIR, os.path.basename(src) + ".o")
        for ext in ("", ".d", ".resources.json"):
            assert os.path.exists(obj + ext), obj + ext
        assert not _lib._stale(obj), obj

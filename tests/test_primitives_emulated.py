"""tests/test_gpu_primitives.py on the CPU: the same translation unit (tests/gpu_prims/prims.hip) compiled by g++ over tests/hipemu, i.e. over the scalar twin of
cfhd_gfx950.h that every emulated test of the kernels stands on.  The arbiter is the same numpy statement of each primitive, so the twin and the hardware header are
held to one definition: a twin that drifts from the header is found here, a header that drifts from its comments on the GPU."""
import pytest
import test_gpu_primitives as P


def _cases(module):
    """Every test of the module, once per value of its (single) parametrize mark."""
    out = []
    for name in sorted(n for n in dir(module) if n.startswith("test_") and callable(getattr(module, n))):
        marks = [m for m in getattr(getattr(module, name), "pytestmark", []) if m.name == "parametrize"]
        if not marks: out.append(pytest.param(module, name, {}, id=name)); continue
        assert len(marks) == 1 and "," not in marks[0].args[0]
        for v in marks[0].args[1]: out.append(pytest.param(module, name, {marks[0].args[0]: v}, id="%s[%s]" % (name, v)))
    return out


@pytest.mark.parametrize("module,name,kw", _cases(P))
def test_on_the_scalar_twin(module, name, kw):
    P.EMULATED = True
    try:
        getattr(module, name)(**kw)
    finally:
        P.EMULATED = False

"""No GPU: the per-map chi^2 and robust polish entry points are built, declared and bound (lsfm_map_chi2, lsfm_gn_polish_robust,
Context.map_chi2, Context.gn_polish_robust), and the C ABI refuses bad arguments before it needs a device."""
import ctypes as C

import pytest


def _lib():
    from linearsfm_amd import api
    return api, api.lib()


def test_library_exports_chi2_and_robust_polish():
    api, L = _lib()
    for name in ("lsfm_map_chi2", "lsfm_gn_polish_robust"):
        assert hasattr(L, name)
        assert name in api.EXPORTS
    assert callable(getattr(api.Context, "map_chi2", None))
    assert callable(getattr(api.Context, "gn_polish_robust", None))


@pytest.mark.parametrize("kind,c", [(3, 1.0), (-1, 1.0), (1, 0.0), (2, -2.0), (1, float("nan")), (2, float("inf"))])
def test_robust_polish_refuses_bad_kind_or_threshold(kind, c):
    api, L = _lib()
    m = api.LsfmMap()
    obj, gn = (C.c_double * 2)(), (C.c_double * 2)()
    # (no context: the arguments are checked first, so a bad kind / threshold is LSFM_ERR_ARG on any machine)
    assert L.lsfm_gn_polish_robust(None, C.byref(m), 1, 0, C.byref(m), 1, kind, c, obj, gn, None, None, None) == -1


def test_chi2_refuses_missing_output():
    api, L = _lib()
    m = api.LsfmMap()
    assert L.lsfm_map_chi2(None, C.byref(m), 1, 0, C.byref(m), None, None) == -1

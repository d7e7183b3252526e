"""The Python wrappers on the host seam, without a GPU: every single defect of tests/seam_cases.py is refused with the exception class
and the whole message it always had, and leaves every argument as it was; the valid call of every wrapper reaches the library
(ctypes checks the argument count and types against _lib.SIGNATURES before the C function runs) and, without a device, is refused
there with LSF_ERR_NO_DEVICE; and _lib.SIGNATURES is the table it was when every _device entry was written out by hand."""
import numpy as np
import pytest

import seam_cases as C

HOST_CASES = [(w, did, patch, exc, msg) for w in C.WRAPPERS for did, patch, exc, msg in C.host_defects(w)]


@pytest.mark.parametrize("w,did,patch,exc,msg", HOST_CASES, ids=[f"{c[0].name}-{c[1]}" for c in HOST_CASES])
def test_a_single_defect_is_refused_with_the_message_it_always_had(w, did, patch, exc, msg):
    import levelsetfortran_amd as lsf

    if "tensor" in did:
        pytest.importorskip("torch")
    kw = C.apply(w.valid(C.Make("np")), patch)
    before = C.freeze(kw)
    with pytest.raises(exc) as e:
        getattr(lsf, w.name)(**kw)
    assert type(e.value) is exc and str(e.value) == msg
    assert C.freeze(kw) == before


def test_the_table_holds_every_defect_the_wrappers_share():
    ids = {f"{w.name}-{did}" for w, did, *_ in HOST_CASES}
    assert len(ids) == len(HOST_CASES) > 400
    for want in ("narrowBand-phiNB-dtype", "measureBand-mask-missing", "measureBand-xLo-two", "measureBand-xLo-nan", "measureBand-dx-0",
                 "measureBand-dx-inf", "measureBand-dx-nan", "measureBand-iso-nan", "samplePoints-order-name", "advectField-scheme-name",
                 "advectField-arith-name", "advectField-velocity-pair", "advectPoints-velocity-pair", "samplePoints-pts-not-n-by-3",
                 "castRays-dir-c-ordered", "correctField-rad-length", "cutCellsBand-az-read-only", "cutCellsBand-ay-dtype", "cutCellsBand-bx-dtype",
                 "cutCellsBand-bz-dtype", "labelBand-label-list", "extendField-phi-shape",
                 "evolveBandCurv-u-c-ordered", "curvatureBand-gmag-tensor"):
        assert want in ids, want


@pytest.mark.parametrize("w", C.WRAPPERS, ids=[w.name for w in C.WRAPPERS])
def test_the_valid_call_reaches_the_library(w):
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    if _lib.load().lsf_device_count() > 0:
        pytest.skip("a GPU is present")
    kw = w.valid(C.Make("np"))
    before = C.freeze(kw)
    with pytest.raises(lsf.LsfError) as e:
        getattr(lsf, w.name)(**kw)
    assert e.value.code == _lib.LSF_ERR_NO_DEVICE
    assert C.freeze(kw) == before


def test_a_stacked_velocity_is_three_fields():
    """advectPoints takes the velocity's three entries, whatever holds them: one (3, nx+1, ny+1, nz+1) array whose entries are
    Fortran-ordered passes every check like the tuple of its entries (and is no tuple whose truth could be asked for)"""
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    w = next(w for w in C.WRAPPERS if w.name == "advectPoints")
    kw = w.valid(C.Make("np"))
    stacked = np.zeros(C.SHAPE + (3,), order="F").transpose(3, 0, 1, 2)
    for i, f in enumerate(kw["velocity"]):
        stacked[i] = f
    assert all(stacked[i].flags.f_contiguous for i in range(3))
    if _lib.load().lsf_device_count() > 0:
        want, got = lsf.advectPoints(**kw), lsf.advectPoints(**dict(kw, velocity=stacked))
        assert got.pts.tobytes() == want.pts.tobytes() and got.status.tobytes() == want.status.tobytes() and got.info == want.info
    else:
        with pytest.raises(lsf.LsfError) as e:
            lsf.advectPoints(**dict(kw, velocity=stacked))
        assert e.value.code == _lib.LSF_ERR_NO_DEVICE


def test_a_numpy_call_does_not_import_torch():
    """In a fresh interpreter with the library's own torch-first import out of the way: the wrappers and the seam helper import torch
    on the device seam only."""
    import subprocess
    import sys

    code = ("import sys, numpy as np\n"
            "from levelsetfortran_amd import _lib\n"
            "import levelsetfortran_amd as lsf\n"
            "class Lib:\n"
            "    def __getattr__(self, name):\n"
            "        return lambda *a: 0\n"
            "_lib.load = lambda: Lib()\n"
            "phi = np.ones((6, 5, 4), order='F'); m = np.ones((6, 5, 4), np.int32, order='F')\n"
            "pts = np.asfortranarray(np.full((3, 3), 0.5))\n"
            "lsf.narrowBand(5, 4, 3, 0.25, phi, m, m)\n"
            "lsf.measureBand(phi, m, 5, 4, 3, 0.25, (0, 0, 0))\n"
            "lsf.samplePoints(phi, 5, 4, 3, 0.25, (0, 0, 0), pts, mask=m)\n"
            "lsf.advectPoints(pts, 5, 4, 3, 0.25, (0, 0, 0), 0.01, 1, velocity=(phi, phi, phi))\n"
            "assert 'torch' not in sys.modules, 'torch was imported'\n")
    from conftest import ROOT

    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def _type_name(t):
    return None if t is None else t.__name__


def test_signatures_are_what_they_were_when_written_out_by_hand():
    from levelsetfortran_amd import _lib

    got = {name: (_type_name(res), [_type_name(a) for a in args]) for name, (res, args) in _lib.SIGNATURES.items()}
    assert sorted(got) == sorted(SIGNATURES)
    for name in SIGNATURES:
        assert got[name] == SIGNATURES[name], name


I, D, V = "c_int", "c_double", "c_void_p"
PI, PD, PL, PBOX, I3 = "LP_c_int", "LP_c_double", "LP_c_long", "LP_LsfBox", "c_int_Array_3"
S, UL, PV = "c_char_p", "c_ulong", "LP_c_void_p"  # (ctypes' names on LP64: c_size_t and c_uint64 are c_ulong, c_int64 is c_long)
SIGNATURES = {
    "lsf_version": (I, []),
    "lsf_last_error": (S, []),
    "lsf_device_count": (I, []),
    "lsf_set_device": (I, [I]),
    "lsf_release_workspace": (I, []),
    "lsf_skew_wide_fits": (I, [I, I, I]),
    "lsf_profile": (I, [I]),
    "lsf_copy_bandwidth": (I, [UL, I, PD]),
    "lsf_profile_kernel": (S, []),
    "lsf_profile_get": (I, [PD, PD, PD, PL, PI]),
    "lsf_reinit": (I, [V, I, I, I, I, D, D, D, I, PI, V, I]),
    "lsf_reinit_device": (I, [V, V, I, I, I, I, D, D, D, I, I, PI, V, I, V]),
    "lsf_reinit_band": (I, [V, V, I, I, I, I, D, D, D, I, PI, V, I]),
    "lsf_reinit_band_device": (I, [V, V, V, I, I, I, I, D, D, D, I, PI, V, I, V]),
    "lsf_minmax": (I, [V, V, V, I, I, I, I, D, D, D, I, PI, V, I]),
    "lsf_minmax_device": (I, [V, V, V, I, I, I, I, D, D, D, I, PI, V, I, V]),
    "lsf_narrowband": (I, [V, V, V, I, I, I, D]),
    "lsf_narrowband_device": (I, [V, V, V, I, I, I, D, V]),
    "lsf_phi0": (I, [V, I, I, I, D, V, V, V, V, I, V, I]),
    "lsf_phi0_device": (I, [V, I, I, I, D, V, V, V, V, I, V, I, V]),
    "lsf_mesh_check": (I, [V, I, V, I, V, PD]),
    "lsf_mesh_distance": (I, [V, I, I, I, D, V, V, I, V, I, D, I, V]),
    "lsf_mesh_distance_device": (I, [V, I, I, I, D, V, V, I, V, I, D, I, V, V]),
    "lsf_distance_fill": (I, [V, V, I, I, I, D, D, I, PI, V, I, PL]),
    "lsf_distance_fill_device": (I, [V, V, I, I, I, D, D, I, PI, V, I, PL, V]),
    "lsf_extend_field": (I, [V, V, V, I, I, I, D, D, I, PI, V, I, V]),
    "lsf_extend_field_device": (I, [V, V, V, I, I, I, D, D, I, PI, V, I, V, V]),
    "lsf_extend_field_band": (I, [V, V, V, V, I, I, I, D, D, I, PI, V, I, V]),
    "lsf_extend_field_band_device": (I, [V, V, V, V, I, I, I, D, D, I, PI, V, I, V, V]),
    "lsf_advect_field": (I, [V, V, V, V, V, I, I, I, D, D, I, I, I, PI, PD, V, I]),
    "lsf_advect_field_device": (I, [V, V, V, V, V, I, I, I, D, D, I, I, I, PI, PD, V, I, V]),
    "lsf_advect_field_band": (I, [V, V, V, V, V, V, I, I, I, D, D, I, I, I, PI, PD, V, I, V, PD]),
    "lsf_advect_field_band_device": (I, [V, V, V, V, V, V, I, I, I, D, D, I, I, I, PI, PD, V, I, V, PD, V]),
    "lsf_curvature_band": (I, [V, V, V, V, V, I, I, I, D, D, V, PD]),
    "lsf_curvature_band_device": (I, [V, V, V, V, V, I, I, I, D, D, V, PD, V]),
    "lsf_measure_band": (I, [V, V, V, V, I, I, I, D, V, D, V, V]),
    "lsf_measure_band_device": (I, [V, V, V, V, I, I, I, D, V, D, V, V, V]),
    "lsf_cut_cells_band": (I, [V, V, I, I, I, D, D, V, V, V, V, V, V, V, V, V, V]),
    "lsf_cut_cells_band_device": (I, [V, V, I, I, I, D, D, V, V, V, V, V, V, V, V, V, V, V]),
    "lsf_sample_points": (I, [V, V, V, I, I, I, D, V, V, I, I, D, I, D, V, V, V, V, V, V]),
    "lsf_sample_points_device": (I, [V, V, V, I, I, I, D, V, V, I, I, D, I, D, V, V, V, V, V, V, V]),
    "lsf_cast_rays": (I, [V, V, V, I, I, I, D, V, V, V, I, I, D, D, D, D, D, D, D, I, I, V, V, V, V, V, V]),
    "lsf_cast_rays_device": (I, [V, V, V, I, I, I, D, V, V, V, I, I, D, D, D, D, D, D, D, I, I, V, V, V, V, V, V, V]),
    "lsf_advect_points": (I, [V, V, V, V, V, V, I, I, I, D, V, V, I, I, I, D, I, V, PD, V]),
    "lsf_advect_points_device": (I, [V, V, V, V, V, V, I, I, I, D, V, V, I, I, I, D, I, V, PD, V, V]),
    "lsf_correct_field": (I, [V, V, I, I, I, D, V, V, V, I, D, V, PD, V]),
    "lsf_correct_field_device": (I, [V, V, I, I, I, D, V, V, V, I, D, V, PD, V, V]),
    "lsf_reseed_points": (I, [V, V, I, I, I, D, V, V, V, I, I, D, D, D, I, I, D, UL, V, PI, V]),
    "lsf_reseed_points_device": (I, [V, V, I, I, I, D, V, V, V, I, I, D, D, D, I, I, D, UL, V, PI, V, V]),
    "lsf_reseed_get": (I, [V, V, V]),
    "lsf_reseed_get_device": (I, [V, V, V, V]),
    "lsf_label_band": (I, [V, V, V, I, I, I, D, I, I, V, I, PL, V]),
    "lsf_label_band_device": (I, [V, V, V, I, I, I, D, I, I, V, I, PL, V, V]),
    "lsf_evolve_band": (I, [V, V, V, V, V, V, I, I, I, D, D, I, I, I, D, I, I, D, I, PI, PD, V, I, V, PD]),
    "lsf_evolve_band_device": (I, [V, V, V, V, V, V, I, I, I, D, D, I, I, I, D, I, I, D, I, PI, PD, V, I, V, PD, V]),
    "lsf_evolve_band_curv": (I, [V, V, V, V, V, V, I, I, I, D, D, I, I, I, D, I, I, D, I, D, D, PI, PD, PD, V, I, V, PD]),
    "lsf_evolve_band_curv_device": (I, [V, V, V, V, V, V, I, I, I, D, D, I, I, I, D, I, I, D, I, D, D, PI, PD, PD, V, I, V, PD, V]),
    "lsf_extract_surface": (I, [V, I, I, I, D, V, D, PI, PI, V]),
    "lsf_extract_surface_device": (I, [V, I, I, I, D, V, D, PI, PI, V, V]),
    "lsf_extract_get": (I, [V, V]),
    "lsf_extract_get_device": (I, [V, V, V]),
    "lsf_stl_write": (I, [S, V, I, V, I]),
    "lsf_advect_nodes": (I, [V, V, I, I, I, D, V, V, I, I]),
    "lsf_advect_nodes_device": (I, [V, V, I, I, I, D, V, V, I, I, V]),
    "lsf_mirror": (I, [I]),
    "lsf_mirror_sync": (I, [V]),
    "lsf_mirror_forget": (I, [V]),
    "lsf_snapshot": (I, [V, V, I, I, I]),
    "lsf_sumsq_diff": (I, [V, V, I, I, I, PD]),
    "lsf_write_vti": (I, [S, V, I, I, I, D, V]),
    "lsf_stl_read": (I, [S, PI, PI]),
    "lsf_stl_get": (I, [V, V]),
    "lsf_box_reserve": (I, [V, UL]),
    "lsf_reinit_multi": (I, [V, I, I, I, I, D, D, D, I, V, I, V, PI, V, I]),
    "lsf_reinit_multi_f32": (I, [V, I, I, I, I, D, D, D, I, V, I, V, PI, V, I]),
    "lsf_multi_create": (I, [I, I, I, V, I, V, I, PV]),
    "lsf_multi_destroy": (I, [V]),
    "lsf_multi_block": (I, [V, I, V, V, V, V, PI]),
    "lsf_multi_scatter": (I, [V, V]),
    "lsf_multi_upload_block": (I, [V, I, V]),
    "lsf_multi_run": (I, [V, I, D, D, D, I, PI, V, I]),
    "lsf_multi_gather": (I, [V, V]),
    "lsf_slabs_info": (I, [PI, PI, PI, PI, PD]),
    "lsf_peer_selftest": (I, [I, I, PI]),
    "lsf_multi_defaults_get": (I, [PI, PI]),
    "lsf_multi_defaults": (I, [I, I]),
    "lsf_multi_configure": (I, [V, I, I]),
    "lsf_multi_info": (I, [V, PI, PI, PI, PI, PD, PD, PD, PI]),
    "lsf_jacobi_sweep_box": (I, [V, V, V, PBOX, I3, I3, D, D, I, V, V]),
    "lsf_bc_box": (I, [V, V, PBOX, I3, I3, D, V, V]),
    "lsf_sumsq_begin": (I, [V]),
    "lsf_sumsq_end": (I, [V]),
    "lsf_pack_boxes": (I, [V, PBOX, I, V, V, V, V]),
    "lsf_unpack_boxes": (I, [V, PBOX, I, V, V, V, V]),
    "lsf_pack_boxes_f32": (I, [V, PBOX, I, V, V, V, V]),
    "lsf_unpack_boxes_f32": (I, [V, PBOX, I, V, V, V, V]),
    "lsf_pack_box": (I, [V, PBOX, I3, I3, V, V]),
    "lsf_unpack_box": (I, [V, PBOX, I3, I3, V, V]),
    "lsf_reinit_f32": (I, [V, I, I, I, I, D, D, D, I, PI, V, I]),
    "lsf_reinit_f32_device": (I, [V, V, I, I, I, I, D, D, D, I, PI, V, I, V]),
    "lsf_jacobi_sweep_box_f32": (I, [V, V, V, PBOX, I3, I3, D, D, I, V, V]),
    "lsf_bc_box_f32": (I, [V, V, PBOX, I3, I3, D, V, V]),
    "lsf_pack_box_f32": (I, [V, PBOX, I3, I3, V, V]),
    "lsf_unpack_box_f32": (I, [V, PBOX, I3, I3, V, V]),
}

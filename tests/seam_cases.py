"""One valid call of every Python wrapper that takes fields or points, and the single defects that each must refuse: the table
behind tests/test_python_seam_cpu.py (host seam) and tests/test_gpu_python_seam.py (device seam).

Grid: nx, ny, nz = 5, 4, 3 -- a numpy field is (6, 5, 4) Fortran-ordered, a tensor (4, 5, 6) contiguous, so neither passes for the
other.  Three points.  Every wrapper is called by keyword, so a case is a dictionary of arguments and a defect replaces one entry.
The messages are literals: they are what the wrappers raised before the seam helper existed.
"""
from typing import NamedTuple

import numpy as np

N = (5, 4, 3)
SHAPE = (6, 5, 4)
DX = 0.25
LO = (0.0, 0.0, 0.0)
GRID = dict(nx=5, ny=4, nz=3)
_AX = [np.arange(s) * DX for s in SHAPE]
_X, _Y, _Z = np.meshgrid(*_AX, indexing="ij")
PHI = np.asfortranarray(_X + 0.5 * _Y - 0.25 * _Z - 0.7)  # a plane through the grid: every band holds cells
PTS = np.asfortranarray(np.array([[0.30, 0.40, 0.20], [0.70, 0.55, 0.35], [0.95, 0.30, 0.50]]))
DIR = np.asfortranarray(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, 0.5, 0.25]]))
RAD = np.array([0.05, -0.05, 0.1])
# a tetrahedron inside the grid, outward normals (1-based connectivity, as stlRead returns it)
SURF_X = np.asfortranarray(np.array([[0.3, 0.3, 0.2], [0.9, 0.3, 0.2], [0.5, 0.8, 0.2], [0.5, 0.4, 0.6]]))
SURF_E = np.asfortranarray(np.array([[1, 3, 2], [1, 2, 4], [2, 3, 4], [3, 1, 4]], dtype=np.int32))

FINITE_XLO = "xLo must hold 3 finite values"
FINITE_DX = "dx must be finite and > 0"
ISO = "iso must be finite"
GRID_MSG = "nx, ny, nz must be >= 1"
ORDER = "order must be 'linear' or 'cubic'"
SCHEME = "scheme must be 'rk3' or 'euler'"
ARITH = "arith must be 'strict' or 'fast'"
VELOCITY = "velocity must be a 3-tuple (u, v, w) of fields"
KINDS = " must all be numpy arrays or all be CUDA tensors"
LONG_KINDS = " must all be numpy arrays (host seam) or all be torch CUDA tensors (device seam)"


class Make:
    """The arrays of a valid call, as numpy arrays (kind "np") or CUDA tensors (kind "cuda") holding the same bytes"""

    def __init__(self, kind):
        self.kind = kind

    def field(self, a):
        a = np.asfortranarray(a)
        if self.kind == "np":
            return a.copy(order="F")
        import torch

        return torch.from_numpy(np.ascontiguousarray(a.T)).to("cuda")  # (nz+1, ny+1, nx+1), i the unit-stride axis

    def f64(self, fill=None):
        return self.field(PHI if fill is None else np.full(SHAPE, float(fill)))

    def i32(self, fill=1):
        return self.field(np.full(SHAPE, fill, dtype=np.int32))

    def pts(self, a=PTS):
        if self.kind == "np":
            return a.copy(order="F")
        import torch

        return torch.from_numpy(np.ascontiguousarray(a.T)).to("cuda").t()  # (n, 3) in Fortran order

    def vec(self, a=RAD):
        if self.kind == "np":
            return a.copy()
        import torch

        return torch.from_numpy(a.copy()).to("cuda")

    def uvw(self):
        return (self.f64(0.5), self.f64(-0.25), self.f64(0.125))


class Field(NamedTuple):
    path: tuple  # ("phi",) or ("velocity", 0)
    name: str  # as the messages call it
    dtype: str  # "float64" / "int32"


class Points(NamedTuple):
    path: tuple
    name: str
    count: str  # "npts" / "nrays"
    shape_msg: str = ""  # where the wrapper words the shape error itself


class Wrapper(NamedTuple):
    name: str
    valid: object  # Make -> dict of keyword arguments
    anchor: tuple  # path of the array that decides the seam
    fields: tuple = ()
    points: tuple = ()
    kind_msg: str = ""  # the subject of the "all one kind" message; "" where the wrapper has none and the field check answers
    one_device_msg: str = ""
    scalars: dict = {}  # xlo / dx / iso / grid: message; names: {argument: message}
    extra: tuple = ()  # (id, {argument: value or callable(valid arguments)}, exception, message)
    skip: frozenset = frozenset()  # (field name, defect id) pairs the generic table leaves out
    device: bool = True  # has a device seam
    devices_after: str = ""  # "points" / "fields": what the wrapper checks before it compares the devices of its tensors
    device_extra: tuple = ()  # extra's counterpart for a call on CUDA tensors


def F(*path_name_dtype):
    return tuple(Field((p,) if isinstance(p, str) else p, n, d) for p, n, d in path_name_dtype)


_UVW = ((("velocity", 0), "u", "float64"), (("velocity", 1), "v", "float64"), (("velocity", 2), "w", "float64"))
_TRANSPORT_NAMES = {"scheme": SCHEME, "arith": ARITH}
_NO_TRANSPORT = "give velocity=(u, v, w), speed=F, or both"
_BAND_MASK = "mask must be an int32 field of phi's shape"


def _transport(m, **more):
    return dict(phi=m.f64(), **GRID, dx=DX, dt=0.01, steps=1, velocity=m.uvw(), speed=m.f64(0.1), **more)


def _velocity_cases(msg):
    return (("velocity-pair", {"velocity": lambda kw: kw["velocity"][:2]}, ValueError, msg),
            ("velocity-hole", {"velocity": lambda kw: (kw["velocity"][0], None, kw["velocity"][2])}, ValueError, msg))


WRAPPERS = (
    Wrapper("narrowBand", lambda m: dict(**GRID, dx=DX, phi=m.f64(), phiNB=m.i32(0), phiSB=m.i32(0)), ("phi",),
            F(("phi", "phi", "float64"), ("phiNB", "phiNB", "int32"), ("phiSB", "phiSB", "int32"))),
    Wrapper("minmaxFlow", lambda m: dict(phi=m.f64(), phiNB=m.i32(), phiSB=m.i32(), **GRID, iter=1, dx=DX, h1=0.01), ("phi",),
            F(("phi", "phi", "float64"), ("phiNB", "phiNB", "int32"), ("phiSB", "phiSB", "int32"))),
    Wrapper("reinitBand", lambda m: dict(phi=m.f64(), mask=m.i32(), **GRID, iter=0, dx=DX, h=0.01), ("phi",),
            F(("phi", "phi", "float64"), ("mask", "mask", "int32")),
            extra=(("mask-missing", {"mask": None}, TypeError, "mask must be a numpy array of int32"),
                   ("phiS-on-the-host", {"phiS": lambda kw: kw["phi"].copy(order="F")}, ValueError, "phiS is only available on the device seam"))),
    Wrapper("phi0Init", lambda m: dict(phi=m.f64(), **GRID, dx=DX, xLo=LO, minX=SURF_X.min(axis=0), maxX=SURF_X.max(axis=0),
                                       surfX=SURF_X.copy(order="F"), surfElem=SURF_E.copy(order="F")), ("phi",),
            F(("phi", "phi", "float64"))),
    Wrapper("meshDistance", lambda m: dict(phi=m.f64(), **GRID, dx=DX, xLo=LO, surfX=SURF_X.copy(order="F"), surfElem=SURF_E.copy(order="F")),
            ("phi",), F(("phi", "phi", "float64")), scalars=dict(xlo="xLo must hold 3 values", dx="dx must be > 0"),
            extra=(("width", {"width": 1.0}, ValueError, "width must be finite and >= 1.5 (cells)"),)),
    Wrapper("distanceFill", lambda m: dict(phi=m.f64(), **GRID, dx=DX, mask=m.i32()), ("phi",),
            F(("phi", "phi", "float64"), ("mask", "mask", "int32")),
            extra=(("neither", {"mask": None}, ValueError, "give exactly one of band= (cells; freezes |phi| < band*dx) and mask= (int32; freezes mask == 1)"),
                   ("both", {"band": 2.0}, ValueError, "give exactly one of band= (cells; freezes |phi| < band*dx) and mask= (int32; freezes mask == 1)"))),
    Wrapper("extendField", lambda m: dict(q=m.f64(2.0), phi=m.f64(), **GRID, dx=DX, mask=m.i32()), ("q",),
            F(("q", "q", "float64"), ("phi", "phi", "float64"), ("mask", "mask", "int32")),
            kind_msg="q, phi and mask" + LONG_KINDS, one_device_msg="q, phi and mask must live on one device", devices_after="fields",
            device_extra=(("phi-missing", {"phi": None}, TypeError, "q, phi and mask" + LONG_KINDS),),
            extra=(("neither", {"mask": None}, ValueError, "give exactly one of band= (cells; freezes |phi| < band*dx) and mask= (int32; freezes mask == 1)"),)),
    Wrapper("extendFieldBand", lambda m: dict(q=m.f64(2.0), phi=m.f64(), mask=m.i32(), dx=DX, known=m.i32(0)), ("q",),
            F(("q", "q", "float64"), ("phi", "phi", "float64"), ("mask", "mask", "int32"), ("known", "known", "int32")),
            kind_msg="q, phi, mask and known" + LONG_KINDS, one_device_msg="q, phi, mask and known must live on one device",
            devices_after="fields", device_extra=(("phi-missing", {"phi": None}, TypeError, "q, phi, mask and known" + LONG_KINDS),),
            scalars=dict(dx=FINITE_DX), skip=frozenset({("q", "shape"), ("q", "list")}),  # the grid size is q's shape
            extra=(("mask-missing", {"mask": None}, ValueError, "mask (int32) must be a field of phi's shape"),
                   ("q-list", {"q": lambda kw: kw["q"].tolist()}, TypeError, "q must be a numpy array of float64 or a CUDA tensor of torch.float64"),
                   ("q-flat", {"q": lambda kw: kw["q"].ravel(order="F")}, ValueError, "q must be a 3-D field: the grid size is taken from its shape"),
                   ("known-and-band", {"band": 2.0}, ValueError,
                    "give exactly one of known= (int32; freezes the list cells with known == 1) and band= (cells; freezes |phi| < band*dx)"),
                   ("q-is-phi", {"phi": lambda kw: kw["q"]}, ValueError, "q and phi must be different arrays"),
                   ("max_passes", {"max_passes": 0}, ValueError, "max_passes must be >= 1"))),
    Wrapper("advectField", _transport, ("phi",), F(("phi", "phi", "float64"), *_UVW, ("speed", "speed", "float64")),
            kind_msg="phi, velocity and speed" + KINDS, one_device_msg="phi, velocity and speed must live on one device",
            scalars=dict(names=_TRANSPORT_NAMES),
            extra=_velocity_cases(VELOCITY) + (("no-transport", {"velocity": None, "speed": None}, ValueError, _NO_TRANSPORT),)),
    Wrapper("advectFieldBand", lambda m: _transport(m, mask=m.i32()), ("phi",),
            F(("phi", "phi", "float64"), ("mask", "mask", "int32"), *_UVW, ("speed", "speed", "float64")),
            kind_msg="phi, mask, velocity and speed" + KINDS, one_device_msg="phi, mask, velocity and speed must live on one device",
            scalars=dict(names=_TRANSPORT_NAMES),
            extra=_velocity_cases(VELOCITY) + (("mask-missing", {"mask": None}, ValueError, _BAND_MASK),
                                               ("no-transport", {"velocity": None, "speed": None}, ValueError, _NO_TRANSPORT))),
    Wrapper("evolveBand", lambda m: _transport(m, mask=m.i32()), ("phi",),
            F(("phi", "phi", "float64"), ("mask", "mask", "int32"), *_UVW, ("speed", "speed", "float64")),
            kind_msg="phi, mask, velocity and speed" + KINDS, one_device_msg="phi, mask, velocity and speed must live on one device",
            scalars=dict(names=_TRANSPORT_NAMES),
            extra=_velocity_cases(VELOCITY) + (("mask-missing", {"mask": None}, ValueError, _BAND_MASK),
                                               ("no-transport", {"velocity": None, "speed": None}, ValueError, _NO_TRANSPORT),
                                               ("ring", {"ring": 9}, ValueError, "ring must be an integer in 1..8"))),
    Wrapper("evolveBandCurv", lambda m: _transport(m, mask=m.i32(), curvature=0.01), ("phi",),
            F(("phi", "phi", "float64"), ("mask", "mask", "int32"), *_UVW, ("speed", "speed", "float64")),
            kind_msg="phi, mask, velocity and speed" + KINDS, one_device_msg="phi, mask, velocity and speed must live on one device",
            scalars=dict(names=_TRANSPORT_NAMES),
            extra=_velocity_cases(VELOCITY) + (("mask-missing", {"mask": None}, ValueError, _BAND_MASK),
                                               ("no-transport", {"velocity": None, "speed": None, "curvature": 0.0}, ValueError,
                                                "give velocity=(u, v, w), speed=F, a curvature > 0, or several of them"),
                                               ("curvature", {"curvature": float("inf")}, ValueError, "curvature must be finite and >= 0"))),
    Wrapper("curvatureBand", lambda m: dict(phi=m.f64(), mask=m.i32(), **GRID, dx=DX, kappa=m.f64(-7.0), gauss=m.f64(-7.0), gmag=m.f64(-7.0)),
            ("phi",), F(("phi", "phi", "float64"), ("mask", "mask", "int32"), ("kappa", "kappa", "float64"), ("gauss", "gauss", "float64"),
                        ("gmag", "gmag", "float64")),
            kind_msg="phi, mask, kappa, gauss and gmag" + KINDS, one_device_msg="phi, mask, kappa, gauss and gmag must live on one device",
            extra=(("mask-missing", {"mask": None}, ValueError, "mask (int32) and kappa (float64) must be fields of phi's shape"),
                   ("clamp", {"clamp": -1.0}, ValueError, "clamp must be finite and >= 0 (0: no clamp)"))),
    Wrapper("measureBand", lambda m: dict(phi=m.f64(), mask=m.i32(), **GRID, dx=DX, xLo=LO, q=m.f64(2.0), cell_area=m.f64(-7.0)), ("phi",),
            F(("phi", "phi", "float64"), ("mask", "mask", "int32"), ("q", "q", "float64"), ("cell_area", "cell_area", "float64")),
            kind_msg="phi, mask, q and cell_area" + KINDS, one_device_msg="phi, mask, q and cell_area must live on one device",
            scalars=dict(xlo=FINITE_XLO, dx=FINITE_DX, iso=ISO),
            extra=(("mask-missing", {"mask": None}, ValueError, "mask (int32) must be a field of phi's shape"),)),
    Wrapper("cutCellsBand", lambda m: dict(phi=m.f64(), mask=m.i32(), **GRID, dx=DX, vof=m.f64(-7.0),
                                           aperture=(m.f64(-7.0), m.f64(-7.0), m.f64(-7.0)), area_vector=(m.f64(-7.0), m.f64(-7.0), m.f64(-7.0))),
            ("phi",), F(("phi", "phi", "float64"), ("mask", "mask", "int32"), ("vof", "vof", "float64"), (("aperture", 0), "ax", "float64"),
                        (("aperture", 1), "ay", "float64"), (("aperture", 2), "az", "float64"), (("area_vector", 0), "bx", "float64"),
                        (("area_vector", 1), "by", "float64"), (("area_vector", 2), "bz", "float64")),
            kind_msg="phi, mask and the outputs" + KINDS, one_device_msg="phi, mask and the outputs must live on one device",
            scalars=dict(dx=FINITE_DX, iso=ISO),
            extra=(("mask-missing", {"mask": None}, ValueError, "mask (int32) must be a field of phi's shape"),
                   ("aperture-pair", {"aperture": lambda kw: kw["aperture"][:2]}, ValueError, "aperture must be a 3-tuple of fields of phi's shape"),
                   ("area_vector-hole", {"area_vector": lambda kw: (kw["area_vector"][0], None, kw["area_vector"][2])}, ValueError,
                    "area_vector must be a 3-tuple of fields of phi's shape"))),
    Wrapper("labelBand", lambda m: dict(phi=m.f64(), mask=m.i32(), **GRID, label=m.i32(-7)), ("phi",),
            F(("phi", "phi", "float64"), ("mask", "mask", "int32"), ("label", "label", "int32")),
            kind_msg="phi, mask and label" + KINDS, one_device_msg="phi, mask and label must live on one device", scalars=dict(iso=ISO),
            extra=(("mask-missing", {"mask": None}, ValueError, "mask and label (int32) must be fields of phi's shape"),
                   ("side", {"side": "left"}, ValueError, 'side must be "inside", "outside" or "both"'),
                   ("comp_cap", {"comp_cap": -1}, ValueError, "comp_cap must be >= 0"))),
    Wrapper("samplePoints", lambda m: dict(phi=m.f64(), **GRID, dx=DX, xLo=LO, pts=m.pts(), mask=m.i32(), q=m.f64(2.0), iters=2), ("phi",),
            F(("phi", "phi", "float64"), ("mask", "mask", "int32"), ("q", "q", "float64")), (Points(("pts",), "pts", "npts"),),
            kind_msg="phi, mask, q and pts" + KINDS, one_device_msg="phi, mask, q and pts must live on one device",
            device_extra=(("pts-missing", {"pts": None}, TypeError, "phi, mask, q and pts" + KINDS),),
            scalars=dict(xlo=FINITE_XLO, dx=FINITE_DX, iso=ISO, grid=GRID_MSG, names={"order": ORDER}),
            extra=(("iters", {"iters": -1}, ValueError, "iters must be >= 0"), ("tol", {"tol": float("nan")}, ValueError, "tol must be finite and >= 0"))),
    Wrapper("castRays", lambda m: dict(phi=m.f64(), **GRID, dx=DX, xLo=LO, org=m.pts(), dir=m.pts(DIR), mask=m.i32(), q=m.f64(2.0)), ("phi",),
            F(("phi", "phi", "float64"), ("mask", "mask", "int32"), ("q", "q", "float64")),
            (Points(("org",), "org", "nrays", "org and dir must have one shape (nrays, 3) with nrays >= 1"),
             Points(("dir",), "dir", "nrays", "org and dir must have one shape (nrays, 3) with nrays >= 1")),
            kind_msg="phi, mask, q, org and dir" + KINDS, one_device_msg="phi, mask, q, org and dir must live on one device",
            device_extra=(("org-missing", {"org": None}, TypeError, "phi, mask, q, org and dir" + KINDS),
                          ("dir-missing", {"dir": None}, TypeError, "phi, mask, q, org and dir" + KINDS)),
            scalars=dict(xlo=FINITE_XLO, dx=FINITE_DX, iso=ISO, grid=GRID_MSG, names={"order": ORDER}),
            extra=(("safety", {"safety": 0.0}, ValueError, "safety must lie in (0, 1]"),
                   ("tmax", {"tmax": 0.0}, ValueError, "tmin must be finite and >= 0, tmax finite and > tmin"))),
    Wrapper("advectPoints", lambda m: dict(pts=m.pts(), **GRID, dx=DX, xLo=LO, dt=0.01, steps=2, velocity=m.uvw(), speed=m.f64(0.1), phi=m.f64(),
                                           mask=m.i32()), ("pts",),
            F(*_UVW, ("phi", "phi", "float64"), ("speed", "speed", "float64"), ("mask", "mask", "int32")), (Points(("pts",), "pts", "npts"),),
            kind_msg="pts and the fields" + KINDS, one_device_msg="pts and the fields must live on one device", devices_after="points",
            scalars=dict(xlo=FINITE_XLO, dx=FINITE_DX, grid=GRID_MSG, names={"order": ORDER, "scheme": SCHEME}),
            extra=_velocity_cases("velocity must be (u, v, w)") + (
                ("no-transport", {"velocity": None, "speed": None, "phi": None}, ValueError, "neither a velocity nor a speed is given"),
                ("speed-without-phi", {"phi": None}, ValueError, "speed and phi are given together"),
                ("steps", {"steps": 0}, ValueError, "steps must be in 1..4096"), ("dt", {"dt": float("nan")}, ValueError, "dt must be finite"))),
    Wrapper("correctField", lambda m: dict(phi=m.f64(), **GRID, dx=DX, xLo=LO, pts=m.pts(), rad=m.vec(), mask=m.i32()), ("phi",),
            F(("phi", "phi", "float64"), ("mask", "mask", "int32")), (Points(("pts",), "pts", "npts"),),
            kind_msg="phi, mask, pts and rad" + KINDS, one_device_msg="phi, mask, pts and rad must live on one device", devices_after="points",
            device_extra=(("pts-missing", {"pts": None}, TypeError, "phi, mask, pts and rad" + KINDS),
                          ("rad-missing", {"rad": None}, TypeError, "phi, mask, pts and rad" + KINDS),
                          ("rad-on-the-host", {"rad": lambda kw: kw["rad"].cpu()}, ValueError, "phi, mask, pts and rad must live on one device")),
            scalars=dict(xlo=FINITE_XLO, dx=FINITE_DX, grid=GRID_MSG),
            extra=(("rad-length", {"rad": np.ones(4)}, ValueError, "rad must have shape (npts,)"),
                   ("rad-dtype", {"rad": np.ones(3, np.float32)}, TypeError, "rad must be a contiguous float64 numpy array"),
                   ("rad-strided", {"rad": np.ones(6)[::2]}, TypeError, "rad must be a contiguous float64 numpy array"),
                   ("slack", {"slack": -1.0}, ValueError, "slack must be finite and >= 0"))),
    Wrapper("seedParticles", lambda m: dict(phi=m.f64(), **GRID, dx=DX, xLo=LO, mask=m.i32(), per_cell=2), ("phi",),
            F(("phi", "phi", "float64"), ("mask", "mask", "int32")), kind_msg="phi, mask, q and pts" + KINDS,
            scalars=dict(xlo=FINITE_XLO, dx=FINITE_DX, grid=GRID_MSG), skip=frozenset({("phi", "shape"), ("mask", "shape")}), device=False,
            extra=(("phi-shape", {"phi": np.zeros((4, 5, 6), order="F")}, ValueError, "phi must be a numpy array of shape (nx+1, ny+1, nz+1)"),)),
    Wrapper("reseedParticles", lambda m: dict(phi=m.f64(), **GRID, dx=DX, xLo=LO, pts=m.pts(), rad=m.vec(), mask=m.i32()), ("phi",),
            F(("phi", "phi", "float64"), ("mask", "mask", "int32")), (Points(("pts",), "pts", "npts"),),
            kind_msg="phi, mask, pts and rad" + KINDS, one_device_msg="phi, mask, pts and rad must live on one device", devices_after="points",
            device_extra=(("rad-on-the-host", {"rad": lambda kw: kw["rad"].cpu()}, ValueError, "phi, mask, pts and rad must live on one device"),),
            scalars=dict(xlo=FINITE_XLO, dx=FINITE_DX, grid=GRID_MSG, names={"order": ORDER}),
            extra=(("rad-length", {"rad": np.ones(4)}, ValueError, "rad must have shape (npts,)"),
                   ("rad-dtype", {"rad": np.ones(3, np.float32)}, TypeError, "rad must be a contiguous float64 numpy array"),
                   ("rad-missing", {"rad": None}, ValueError, "pts and rad are given together"),
                   ("per_cell", {"per_cell": 0}, ValueError, "per_cell must be in 1..4096"),
                   ("radii", {"rmin": 0.6}, ValueError, "0 < rmin <= rmax and rmin < band are required, all finite"))),
    Wrapper("extractSurface", lambda m: dict(phi=m.f64(), **GRID, dx=DX, xLo=LO), ("phi",), F(("phi", "phi", "float64")),
            scalars=dict(xlo="xLo must hold 3 values", dx=FINITE_DX, iso=ISO, grid=GRID_MSG)),
    Wrapper("advectNodes", lambda m: dict(phi=m.f64(), phiSB=m.i32(), **GRID, dx=DX, xLo=LO, surfXX=SURF_X.copy(order="F"), iter=2), ("phi",),
            F(("phi", "phi", "float64"), ("phiSB", "phiSB", "int32")),
            extra=(("surfXX-c-ordered", {"surfXX": np.ascontiguousarray(SURF_X)}, ValueError,
                    "surfXX must be a writeable Fortran-ordered float64 array of shape (nSurfNode, 3)"),)),
)


def get(kw, path):
    v = kw[path[0]]
    return v if len(path) == 1 else v[path[1]]


def put(kw, path, value):
    if len(path) == 1:
        kw[path[0]] = value
    else:
        t = list(kw[path[0]])
        t[path[1]] = value
        kw[path[0]] = tuple(t)


def freeze(v):
    """A value of a call as something `==` compares bit for bit: arrays and tensors by dtype, shape and bytes"""
    if isinstance(v, np.ndarray):
        return ("array", v.dtype.str, v.shape, v.tobytes())
    if type(v).__module__.startswith("torch"):
        return ("tensor", str(v.dtype), tuple(v.shape), v.detach().cpu().contiguous().numpy().tobytes())
    if isinstance(v, (tuple, list)):
        return (type(v).__name__,) + tuple(freeze(x) for x in v)
    if isinstance(v, dict):
        return {k: freeze(x) for k, x in v.items()}
    return repr(v)


def _read_only(a):
    b = a.copy(order="F")
    b.setflags(write=False)
    return b


def _as_tensor(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a))  # a CPU tensor: the wrappers tell the kinds apart before anything else


def host_defects(w):
    """(id, {path: replacement or callable(valid arguments)}, exception, message) for every single defect of a numpy call of `w`"""
    out = []
    for f in w.fields:
        wrong = np.float32 if f.dtype == "float64" else np.int64
        of_dtype = f"{f.name} must be a numpy array of {f.dtype}"
        shape = f"{f.name} must be Fortran-ordered with shape (nx+1, ny+1, nz+1) = (6, 5, 4)"
        generic = [("dtype", lambda a, wrong=wrong: np.asfortranarray(a.astype(wrong)), TypeError, of_dtype),
                   ("shape", lambda a: np.zeros(SHAPE[::-1], a.dtype, order="F"), ValueError, shape),
                   ("c-ordered", lambda a: np.ascontiguousarray(a), ValueError, shape),
                   ("read-only", _read_only, ValueError, f"{f.name} must be writeable (it is INTENT(INOUT) in the reference)"),
                   ("list", lambda a: a.tolist(), TypeError, of_dtype)]
        if f.path != w.anchor:
            generic.append(("tensor", _as_tensor, TypeError, w.kind_msg or of_dtype))
        for did, fn, exc, msg in generic:
            if (f.name, did) not in w.skip:
                out.append((f"{f.name}-{did}", {f.path: (lambda kw, fn=fn, p=f.path: fn(get(kw, p)))}, exc, msg))
    for p in w.points:
        layout = f"{p.name} must be a Fortran-ordered float64 numpy array of shape ({p.count}, 3)"
        out += [(f"{p.name}-not-n-by-3", {p.path: np.zeros((3, 2), order="F")}, ValueError,
                 p.shape_msg or f"{p.name} must have shape ({p.count}, 3) with {p.count} >= 1"),
                (f"{p.name}-c-ordered", {p.path: (lambda kw, p=p: np.ascontiguousarray(get(kw, p.path)))}, TypeError, layout),
                (f"{p.name}-float32", {p.path: (lambda kw, p=p: np.asfortranarray(get(kw, p.path).astype(np.float32)))}, TypeError, layout)]
        if p.path != w.anchor:
            out.append((f"{p.name}-tensor", {p.path: (lambda kw, p=p: _as_tensor(get(kw, p.path)))}, TypeError, w.kind_msg))
    s = w.scalars
    if "xlo" in s:
        out.append(("xLo-two", {("xLo",): (0.0, 0.0)}, ValueError, s["xlo"]))
        if "finite" in s["xlo"]:
            out.append(("xLo-nan", {("xLo",): (0.0, float("nan"), 0.0)}, ValueError, s["xlo"]))
    if "dx" in s:
        out += [(f"dx-{v}", {("dx",): float(v)}, ValueError, s["dx"]) for v in ("0", "inf", "nan")]
    if "iso" in s:
        out.append(("iso-nan", {("iso",): float("nan")}, ValueError, s["iso"]))
    if "grid" in s:
        out.append(("nz-0", {("nz",): 0}, ValueError, s["grid"]))
    for arg, msg in s.get("names", {}).items():
        out.append((f"{arg}-name", {(arg,): "bogus"}, ValueError, msg))
    out += [(did, {(k,): v for k, v in patch.items()}, exc, msg) for did, patch, exc, msg in w.extra]
    return out


def device_defects(w):
    """The same for a call on CUDA tensors: (id, patch, exception, message); a patch value is called with the valid arguments"""
    import torch

    out = []
    floats = [f for f in w.fields if f.dtype == "float64"]
    ints = [f for f in w.fields if f.dtype == "int32"]
    others = [f for f in w.fields if f.path != w.anchor]
    if floats:
        f = floats[0]
        out += [(f"{f.name}-float32", {f.path: (lambda kw, f=f: get(kw, f.path).float())}, TypeError, f"{f.name} must be a CUDA tensor of torch.float64"),
                (f"{f.name}-strided", {f.path: (lambda kw: torch.zeros((4, 5, 12), dtype=torch.float64, device="cuda")[:, :, ::2])}, ValueError,
                 f"{f.name} must be contiguous")]
        f = next(g for g in floats if (g.name, "shape") not in w.skip)
        out.append((f"{f.name}-numpy-shape", {f.path: (lambda kw: torch.zeros(SHAPE, dtype=torch.float64, device="cuda"))}, ValueError,
                    f"{f.name} must have shape (nz+1, ny+1, nx+1) (i is the unit-stride axis)"))
    if ints:
        f = ints[0]
        out.append((f"{f.name}-int64", {f.path: (lambda kw, f=f: get(kw, f.path).long())}, TypeError, f"{f.name} must be a CUDA tensor of torch.int32"))
    if others:
        f = others[0]
        out.append((f"{f.name}-numpy-among-tensors", {f.path: (lambda kw, f=f: np.asfortranarray(get(kw, f.path).cpu().numpy().T))},
                    TypeError if w.kind_msg else AttributeError, w.kind_msg or "'numpy.ndarray' object has no attribute 'is_cuda'"))
        # a CPU tensor among CUDA tensors is of their kind: the comparison of the devices answers, or the field check where it runs first
        if w.one_device_msg and w.devices_after != "fields":
            exc, msg = ValueError, w.one_device_msg
        else:
            exc, msg = TypeError, f"{f.name} must be a CUDA tensor of torch.{f.dtype}"
        out.append((f"{f.name}-on-the-host", {f.path: (lambda kw, f=f: get(kw, f.path).cpu())}, exc, msg))
    for p in w.points:
        layout = f"{p.name} must be a float64 CUDA tensor of shape ({p.count}, 3) in Fortran order (the transpose of a contiguous (3, {p.count}))"
        out.append((f"{p.name}-contiguous", {p.path: (lambda kw, p=p: get(kw, p.path).contiguous())}, TypeError, layout))
        exc, msg = (TypeError, layout) if w.devices_after == "points" else (ValueError, w.one_device_msg)
        out.append((f"{p.name}-on-the-host", {p.path: (lambda kw, p=p: get(kw, p.path).cpu())}, exc, msg))
    out += [(did, {(k,): v for k, v in patch.items()}, exc, msg) for did, patch, exc, msg in w.device_extra]
    return out


def apply(kw, patch):
    """`kw` with the entries of `patch` replaced (a callable is given the valid arguments)"""
    new = dict(kw)
    for path, v in patch.items():
        put(new, path, v(kw) if callable(v) else v)
    return new

"""Parallel- and cone-beam tomography of the contrast phantom or of a labelled voxel volume: the inverse of the projections the package simulates and retrieves.

    fbp(sinogram, angles_deg, ...)      filtered back-projection on the GPU (csrc/fbp.hip, ops.FbpPlan; the contract is in
                                        include/paresis_hip.h): [A, n, m] maps, one per angle -> [n, m, m], a slice per
                                        detector row.  The sinogram holds LINE INTEGRALS IN PIXELS of the slice's voxel: a
                                        map in physical units (phi in radians, -ln T) gives the quantity per voxel length.
                                        filter='hilbert' | 'hilbert-hann': the sinogram is DIFFERENTIAL, d/d(column) of
                                        those integrals per detector pixel, and is back-projected through a Hilbert filter.
    fdk(sinogram, angles_deg, source_px, ...)   FDK of a full-turn cone-beam scan on the virtual detector through the axis
                                        (ops.FdkPlan, k_fdk_backproject): the source source_px voxels from the axis
    forward_project(vol, angles_deg, ...)    the matched pair behind the iterative methods (ops.fbp_project / fbp_adjoint):
    back_project(sinogram, angles_deg, ...)  B^T vol, the exact transpose of fbp's interpolation, and B sinogram, unscaled
    sirt(sinogram, angles_deg, iterations, ..., nonneg)   SIRT and CGLS on min |B^T x - b|: what few angles call for,
    cgls(sinogram, angles_deg, iterations, ...)           where filtered back-projection streaks
    tv(sinogram, angles_deg, iterations, weight, ..., nonneg)   min 0.5 |B^T x - b|^2 + weight TV(x): the model of a piecewise
    tv_objective(vol, sinogram, angles_deg, weight, ...)        constant object such as the phantom (ops.fbp_tv_step)
    delta_volume(vol, energy_keV, voxel_m)   phi = -k * integral(delta) dl  ->  delta = -vol/(k*voxel), k = getk(E)
    mu_volume(vol, voxel_m)                  -ln T = integral(mu) dl         ->  mu = vol/voxel (1/m)
    project(sample, energy_keV, angles_deg, dims, pixel_um)   the sample's ideal sinograms phi and -ln T on the study grid
    scan(experiment, angles_deg, modality, differential, beam)   the real chain once per angle -> sinograms per energy bin
    rotation_center(experiment)                               the detector column of the rotation axis of such a scan
    optical_row(experiment), source_distance(experiment)      the detector row of the optical axis; the source's distance (m)
    save_volume(vol, path, fmt)

By default the beam is treated as parallel.  At the magnification of the shipped experiments (M ~ 1.03) that is the
synchrotron case.  A laboratory source is a point: scan(..., beam='cone') projects a label volume along the rays that diverge
from it (the source at source_distance(experiment) from the rotation axis, the sinogram on the virtual detector through the
axis, whose pixel is the voxel) over a full turn, and reconstruct undoes it by FDK (Feldkamp, Davis, Kress 1984): method
'fbp' on a cone scan.  The contrast phantom's kernel is analytic and parallel; contrast_phantom_volume gives it as a label
volume.  Two samples have a three-dimensional description, projected at Sample.myAngle by
the same model (scikit-image radon of a slice): the contrast phantom (Samples/generateContrastPhantom.py: 13 material
discs on a slice) and a volume of material labels the user brings (Samples/getVolumeFromFile.py: uint8 [n, m, m], from
the sample's myVolumeFile or set as myVolume).  project and scan refuse every other sample.

Differential phase tomography: speckle tracking measures the phase GRADIENT.  scan(modality='phase') integrates each angle's
(dx, dy) into phi (Frankot-Chellappa) and fbp's ramp differentiates it again; scan(..., differential=True) keeps the
gradient across the rotation axis instead -- dy times retrieval.gradient_scale, radians per detector pixel -- and
reconstruct back-projects it through the Hilbert filter: 2|f| = (i 2 pi f) * (-i sgn f / pi), the ramp is the derivative
followed by a Hilbert transform.  No two-dimensional integration, with its mirror extension and its low-frequency errors
along whole rows, is run.

    python -m paresis_amd.main --tomography A [--tomography-modality attenuation|phase [--tomography-differential]]
                               [--tomography-method fbp|sirt|cgls|tv --tomography-iterations K [--tomography-weight W]]
                               [--tomography-beam parallel|cone] ...
"""
import collections
import contextlib
import os

import numpy as np

from . import _lib
from .getk import getk

MODALITIES = ("attenuation", "phase")
BEAMS = ("parallel", "cone")
PHANTOM_FUNCTION = "generateContrastPhantom"
VOLUME_FUNCTION = "getVolumeFromFile"
ROTATABLE_FUNCTIONS = (PHANTOM_FUNCTION, VOLUME_FUNCTION)
_plans = {}
_fdk_plans = {}


def _angles(angles_deg):
    """Angles in degrees, in any array-like form -> a tuple of floats."""
    return tuple(float(a) for a in np.asarray(angles_deg, dtype=np.float64).ravel())


def _sinogram(sinogram, angles_deg):
    """-> (the [A, n, m] tensor, the angles as a tuple of floats), checked on the host."""
    import torch
    from . import ops
    if not isinstance(sinogram, torch.Tensor):
        sinogram = torch.stack(list(sinogram))
    ops._need(sinogram, torch.float32, "sinogram")
    if sinogram.dim() != 3:
        raise ops.PsxError("sinogram must be [A, n, m], got shape %s" % (tuple(sinogram.shape),))
    angles = _angles(angles_deg)
    if len(angles) != sinogram.shape[0]:
        raise ops.PsxError("sinogram holds %d projections, angles_deg %d" % (sinogram.shape[0], len(angles)))
    return sinogram, angles


def _plan(dev, angles, m, center, filter, circle):
    """The module's plan of (device, A, m, angles, center, filter, circle), made on first use."""
    import torch
    from . import ops
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (index, len(angles), m, angles, float(m // 2 if center is None else center), str(filter), bool(circle))
    plan = _plans.get(key)
    if plan is None:
        plan = _plans[key] = ops.FbpPlan(angles, m, center=key[4], filter=filter, circle=circle,
                                         device=torch.device("cuda", index))
    return plan


def fbp(sinogram, angles_deg, center=None, filter='ramp', circle=True):
    """Filtered back-projection of an [A, n, m] float32 CUDA tensor (or a sequence of A n x m maps, as retrieval.retrieve and
    retrieval.paganin return them) taken at angles_deg (A angles in degrees, any values) -> the [n, m, m] float32 volume on
    the same device: vol[r] is the slice of detector row r in the orientation of contrast_phantom_slices.  center: the
    detector column of the rotation axis (None: m // 2, scikit-image radon's; rotation_center for a scan).  filter:
    'ramp', 'hann' or 'none'; 'hilbert' or 'hilbert-hann' (the Hilbert filter, alone or under the Hann window): the sinogram
    is then the DERIVATIVE of those line integrals along axis 2, per detector pixel, and the volume is what 'ramp' / 'hann'
    give on the integrals themselves, to discretisation.  A constant offset of such a sinogram is not removed exactly.
    circle: zero outside the inscribed circle.  One plan per (device, A, m, angles, center, filter, circle) is kept for the
    process's lifetime."""
    from . import ops
    sinogram, angles = _sinogram(sinogram, angles_deg)
    return ops.fbp(sinogram, _plan(sinogram.device, angles, int(sinogram.shape[2]), center, filter, circle))


def fdk(sinogram, angles_deg, source_px, center=None, row_center=None, filter='ramp', circle=True):
    """FDK reconstruction of an [A, n, m] float32 CUDA tensor (or a sequence of A n x m maps): a cone-beam scan on the
    virtual detector through the rotation axis (pixel = voxel) at angles_deg, A angles in degrees that cover a full turn
    evenly, from a point source source_px voxels from the axis (m <= source_px <= 1e30) -> the [n, m, m] float32 volume in
    fbp's orientation and fbp's unit.  center: the axis's detector column (None: m // 2; rotation_center for a scan);
    row_center: the detector row of the optical axis, any real (None: (n - 1)/2; optical_row for a scan); slice Z lies at
    height Z - row_center.  filter: 'ramp', 'hann' or 'none'.  One plan per (device, A, n, m, angles, source_px, center,
    row_center, filter, circle) is kept for the process's lifetime; it holds the filtered sinogram, A*n*m float32."""
    import torch
    from . import ops
    sinogram, angles = _sinogram(sinogram, angles_deg)
    n, m = int(sinogram.shape[1]), int(sinogram.shape[2])
    dev = sinogram.device
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (index, n, m, angles, float(source_px), float(m // 2 if center is None else center),
           float((n - 1) / 2.0 if row_center is None else row_center), str(filter), bool(circle))
    plan = _fdk_plans.get(key)
    if plan is None:
        plan = _fdk_plans[key] = ops.FdkPlan(angles, n, m, key[4], center=key[5], vcenter=key[6], filter=filter, circle=circle,
                                             device=torch.device("cuda", index))
    return ops.fdk(sinogram, plan)


def forward_project(vol, angles_deg, center=None, circle=True):
    """The [A, n, m] float32 sinogram of an [n, m, m] float32 CUDA volume at angles_deg: B^T vol, the exact transpose of the
    interpolation fbp back-projects with (ops.fbp_project), unscaled -- line integrals in pixels, what fbp consumes.
    circle: only the voxels inside the inscribed circle are projected.  Uses the module's plan with filter 'none'."""
    from . import ops
    import torch
    ops._need(vol, torch.float32, "vol")
    if vol.dim() != 3 or vol.shape[1] != vol.shape[2]:
        raise ops.PsxError("vol must be [n, m, m], got shape %s" % (tuple(vol.shape),))
    return ops.fbp_project(vol, _plan(vol.device, _angles(angles_deg), int(vol.shape[2]), center, 'none', circle))


def back_project(sinogram, angles_deg, center=None, circle=True):
    """B sinogram: the [n, m, m] back-projection of an [A, n, m] sinogram without filter and without the pi/(2A) scale
    (ops.fbp_adjoint), the transpose of forward_project.  Uses the module's plan with filter 'none'."""
    from . import ops
    sinogram, angles = _sinogram(sinogram, angles_deg)
    return ops.fbp_adjoint(sinogram, _plan(sinogram.device, angles, int(sinogram.shape[2]), center, 'none', circle))


def _iterations(iterations):
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
        raise ValueError("iterations must be an integer >= 0, got %r" % (iterations,))
    return int(iterations)


def _problem(sinogram, angles_deg, center, circle, x0):
    """What sirt, cgls and tv iterate on -> (b, the checked [A, n, m] sinogram; the module's 'none' plan for it; x, the
    start: a copy of x0, zeros for None)."""
    import torch
    from . import ops
    b, angles = _sinogram(sinogram, angles_deg)
    n, m = int(b.shape[1]), int(b.shape[2])
    plan = _plan(b.device, angles, m, center, 'none', circle)
    if x0 is None:
        return b, plan, torch.zeros((n, m, m), dtype=torch.float32, device=b.device)
    ops._need(x0, torch.float32, "x0", (n, m, m))
    return b, plan, x0.clone()


def _reciprocal(t):
    """1/t where t > 1e-6, 0 elsewhere."""
    import torch
    return torch.where(t > 1e-6, 1.0 / t, torch.zeros_like(t))


def sirt(sinogram, angles_deg, iterations, center=None, circle=True, nonneg=False, x0=None):
    """`iterations` steps of SIRT on min |B^T x - b| for the [A, n, m] sinogram b (line integrals in pixels, as fbp takes
    them) -> the [n, m, m] float32 volume:  x <- x + Cinv * B(Rinv * (b - B^T x)), then max(x, 0) if nonneg, with
    R = B^T 1 (the ray lengths, with the circle), C = B 1 and Rinv, Cinv their reciprocals where they exceed 1e-6, 0
    elsewhere -- computed once per call.  The two projections are ops.fbp_project and ops.fbp_adjoint on the module's
    'none' plan; the element-wise steps are torch's.  x0: the start, zeros by default (not modified)."""
    import torch
    from . import ops
    iterations = _iterations(iterations)
    b, plan, x = _problem(sinogram, angles_deg, center, circle, x0)
    Rinv = _reciprocal(ops.fbp_project(torch.ones_like(x), plan))
    Cinv = _reciprocal(ops.fbp_adjoint(torch.ones_like(b), plan))
    res, upd = torch.empty_like(b), torch.empty_like(x)
    for _ in range(iterations):
        ops.fbp_project(x, plan, out=res)
        torch.sub(b, res, out=res)
        res.mul_(Rinv)
        ops.fbp_adjoint(res, plan, out=upd)
        x.addcmul_(Cinv, upd)
        if nonneg:
            x.clamp_(min=0)
    return x


def cgls(sinogram, angles_deg, iterations, center=None, circle=True, x0=None):
    """`iterations` steps of CGLS on min |B^T x - b| -> the [n, m, m] float32 volume.  With K = B^T:
    r = b - K x, s = B r, p = s, gamma = |s|^2; per step q = K p, alpha = gamma/|q|^2, x += alpha p, r -= alpha q, s = B r,
    beta = |s|^2/gamma, p = s + beta p.  gamma and |q|^2 are taken PER DETECTOR ROW in float64, so every row is its own
    two-dimensional problem and reconstructs the same alone or in a stack, to rounding; a row whose gamma or |q|^2 is 0
    gets alpha = beta = 0, so a zero sinogram row stays exactly 0.  x0: the start, zeros by default (not modified)."""
    import torch
    from . import ops
    iterations = _iterations(iterations)
    b, plan, x = _problem(sinogram, angles_deg, center, circle, x0)

    def ratio(num, den):                               # float64 [n] -> float32 [n], 0 where either is 0
        ok = (num != 0) & (den != 0)
        return torch.where(ok, num / torch.where(ok, den, torch.ones_like(den)), torch.zeros_like(num)).float()

    r = b.clone() if x0 is None else b - ops.fbp_project(x, plan)
    s = ops.fbp_adjoint(r, plan)
    p = s.clone()
    gamma = s.double().pow(2).sum(dim=(1, 2))
    q = torch.empty_like(b)
    for _ in range(iterations):
        ops.fbp_project(p, plan, out=q)
        alpha = ratio(gamma, q.double().pow(2).sum(dim=(0, 2)))
        x.addcmul_(alpha[:, None, None], p)
        r.addcmul_(alpha[None, :, None], q, value=-1.0)
        ops.fbp_adjoint(r, plan, out=s)
        gamma_new = s.double().pow(2).sum(dim=(1, 2))
        beta = ratio(gamma_new, gamma)
        p.mul_(beta[:, None, None]).add_(s)
        gamma = gamma_new
    return x


def _weight(weight):
    try:
        w = float(weight)
    except (TypeError, ValueError):
        w = float("nan")
    if isinstance(weight, bool) or not np.isfinite(w) or w < 0:
        raise ValueError("weight must be a finite number >= 0, got %r" % (weight,))
    return w


def _lit(m, circle, device):
    """The plan's mask as an [m, m] bool tensor: (i - h)^2 + (j - h)^2 <= h^2, h = m // 2; all true without circle."""
    import torch
    d2 = (torch.arange(m, device=device) - m // 2) ** 2
    return (d2[:, None] + d2[None, :] <= (m // 2) ** 2) if circle else torch.ones((m, m), dtype=torch.bool, device=device)


def tv(sinogram, angles_deg, iterations, weight, center=None, circle=True, nonneg=False, x0=None):
    """`iterations` steps of the primal-dual hybrid gradient method on min 0.5 |B^T x - b|^2 + weight * TV(x) (with x >= 0
    if nonneg) for the [A, n, m] sinogram b -> the [n, m, m] float32 volume; every detector row is its own problem.  TV is
    the isotropic total variation of a slice by forward differences between the voxels inside the circle (all, without
    circle); weight (lambda) is in the sinogram's own unit, finite and >= 0 (ValueError otherwise): 0 leaves least squares.
    The steps are Pock and Chambolle's diagonal preconditioners (alpha = 1), which need no operator norm: s1 = 1/R for the
    data dual y, R = B^T 1; 1/2 for the TV dual p; tau = 1/(C + deg) for x, C = B 1 and deg the voxel's number of
    differences (reciprocals where the sum exceeds 1e-6, 0 elsewhere, so a voxel outside the circle keeps its start).
    Per iteration: q = B^T xbar (ops.fbp_project); y <- (y + s1 (q - b))/(1 + s1) (torch); u = B y (ops.fbp_adjoint); then
    ops.fbp_tv_step, one kernel: p <- the projection of p + grad(xbar)/2 onto |p| <= weight, x <- x - tau (u + grad^T p),
    max(x, 0) if nonneg, xbar <- 2 x_new - x_old.  On the module's 'none' plan.  x0: the start of x and xbar, zeros by
    default (not modified).  Held for the call: nine volume-sized arrays (x, xbar and p = (px, py) twice each -- the step
    reads its neighbours, so they go from one buffer to the other --, u and C) and, besides b, four sinogram-sized ones
    (y, q, s1, 1 + s1)."""
    import torch
    from . import ops
    iterations, weight = _iterations(iterations), _weight(weight)
    b, plan, x = _problem(sinogram, angles_deg, center, circle, x0)
    xbar, xbar_new = x.clone(), torch.ones_like(x)
    q = torch.ones_like(b)
    s1 = _reciprocal(ops.fbp_project(xbar_new, plan))
    c = ops.fbp_adjoint(q, plan)
    den = s1 + 1.0
    y, u = torch.zeros_like(b), torch.empty_like(x)
    px, py, px_new, py_new = torch.zeros_like(x), torch.zeros_like(x), torch.empty_like(x), torch.empty_like(x)
    for _ in range(iterations):
        ops.fbp_project(xbar, plan, out=q)
        q.sub_(b).mul_(s1)
        y.add_(q).div_(den)
        ops.fbp_adjoint(y, plan, out=u)
        ops.fbp_tv_step(plan, weight, nonneg, u, c, x, xbar, xbar_new, px, py, px_new, py_new)
        xbar, xbar_new, px, px_new, py, py_new = xbar_new, xbar, px_new, px, py_new, py
    return x


def tv_objective(vol, sinogram, angles_deg, weight, center=None, circle=True):
    """What tv minimises, per detector row: 0.5 |B^T vol - b|^2 + weight * TV(vol) -> a float64 [n] tensor on the volume's
    device.  The projection is ops.fbp_project's; the differences and the sums are torch's, in float64."""
    import torch
    weight = _weight(weight)
    b, angles = _sinogram(sinogram, angles_deg)
    r = forward_project(vol, angles, center=center, circle=circle).double() - b.double()
    v = vol.double()
    lit = _lit(int(vol.shape[2]), circle, vol.device)
    gx, gy = torch.zeros_like(v), torch.zeros_like(v)
    gx[:, :-1, :] = (v[:, 1:, :] - v[:, :-1, :]) * (lit[:-1, :] & lit[1:, :])
    gy[:, :, :-1] = (v[:, :, 1:] - v[:, :, :-1]) * (lit[:, :-1] & lit[:, 1:])
    return 0.5 * r.pow(2).sum(dim=(0, 2)) + weight * torch.sqrt(gx ** 2 + gy ** 2).sum(dim=(1, 2))


def delta_volume(vol_phi, energy_keV, voxel_m):
    """The refractive index decrement per voxel from the back-projection of a phase sinogram (radians): the chain's phase is
    phi = -k*sum(delta*t) (Sample.setWaveRT), k = getk(E) with the chain's constants, so delta = -vol/(k*voxel_m)."""
    return vol_phi * (-1.0 / (getk(float(energy_keV) * 1e3) * float(voxel_m)))


def mu_volume(vol_logT, voxel_m):
    """The linear attenuation coefficient (1/m) per voxel from the back-projection of a -ln T sinogram: vol/voxel_m."""
    return vol_logT * (1.0 / float(voxel_m))


def _phantom(sample):
    """The sample, if it can be turned: the contrast phantom or a labelled voxel volume."""
    if getattr(sample, "myGeometryFunction", "") not in ROTATABLE_FUNCTIONS:
        raise ValueError("tomography needs a sample whose geometry function is %s (the only ones with a three-dimensional "
                         "description), got %r" % (" or ".join(ROTATABLE_FUNCTIONS), getattr(sample, "myGeometryFunction", "")))
    return sample


def _turn(sample, angle, dims, pixel_um, ov=1):
    sample.myAngle = float(angle)
    sample.getMyGeometry(dims, pixel_um, ov)


def check_diverging(sample):
    """ValueError unless `sample` can be projected from a point source: a label volume."""
    if getattr(sample, "myGeometryFunction", "") != VOLUME_FUNCTION:
        raise ValueError("a diverging beam needs a %s sample (the contrast phantom's kernel is analytic and parallel; "
                         "contrast_phantom_volume gives it as a label volume), got %r"
                         % (VOLUME_FUNCTION, getattr(sample, "myGeometryFunction", "")))


@contextlib.contextmanager
def _diverging(sample, source_distance_m):
    """A context in which `sample` projects from a point source source_distance_m metres from its axis (None: as it is)."""
    if source_distance_m is None:
        yield
        return
    check_diverging(sample)
    before = getattr(sample, "mySourceDistance", None)
    sample.mySourceDistance = float(source_distance_m)
    try:
        yield
    finally:
        sample.mySourceDistance = before


def project(sample, energy_keV, angles_deg, dims, pixel_um, source_distance_m=None):
    """The ideal sinograms of `sample` (an AnalyticalSample with delta / beta at energy_keV whose geometry function is the
    contrast phantom's or getVolumeFromFile) on a dims = (dimX, dimY) grid of pixel_um pixels ->
    {'phi': [A, dimX, dimY] float32 (radians, -k*sum delta*t), 'logT': [A, dimX, dimY] float32 (-ln of the transmitted
    intensity, 2k*sum beta*t)}.  Per angle the sample is turned (myAngle), its geometry rebuilt (psx_contrast_phantom_f32
    or psx_volume_project_u8) and a unit intensity sent through setWaveRT.  The sample is left at its last angle.
    source_distance_m: None for the parallel beam; otherwise a label volume is projected from a point source that many
    metres from its axis (psx_volume_project_cone_u8; its mySourceDistance is set for the call and restored)."""
    import torch
    _phantom(sample)
    dims = (int(dims[0]), int(dims[1]))
    one = None
    phi, logT = [], []
    with _diverging(sample, source_distance_m):
        for angle in _angles(angles_deg):
            _turn(sample, angle, dims, pixel_um)
            if one is None:
                one = torch.ones(dims, dtype=torch.float32, device=sample.geometry_dev().device)
            I, p, _ = sample.setWaveRT(one, energy_keV)
            phi.append(p.to(torch.float32))
            logT.append(-torch.log(I))
    return {'phi': torch.stack(phi), 'logT': torch.stack(logT)}


def rotation_center(experiment):
    """The detector column of the rotation axis of a scan of `experiment`: (dimY // 2 - (ov - 1)/2)/ov, dimY the study
    grid's axis-1 length.  Needs no GPU.

    The phantom and a label volume are projected with scikit-image radon's convention, whose axis is study column c0 = dimY // 2
    (phantom_scalars' center).  The chains keep the study grid up to the detector, which reflect-pads it by 15*ov pixels,
    sums ov x ov blocks and crops 15 detector pixels (Detector.detection): study column x sits at padded column x + 15*ov,
    in block (x + 15*ov) // ov = x // ov + 15, which the crop brings back to x // ov -- pad and crop cancel, and the study
    grid is ov times the detector's, so nothing else is cut.  Detector pixel c therefore covers study columns
    ov*c ... ov*c + ov - 1, whose centre is ov*c + (ov - 1)/2: a point at study coordinate x is at detector coordinate
    (x - (ov - 1)/2)/ov.  With ov = 2 and dimY = 2*m that is m/2 - 0.25: a quarter of a pixel off m // 2."""
    ov = int(experiment.exp_dict['overSampling'])
    dimY = int(experiment.exp_dict['studyDimensions'][1])
    return (dimY // 2 - (ov - 1) / 2.0) / ov


def optical_row(experiment):
    """The detector row of the optical axis of a scan of `experiment`: rotation_center's formula on the study grid's axis-0
    length, (dimX // 2 - (ov - 1)/2)/ov.  The projectors put height 0 on study row dimX // 2.  Needs no GPU."""
    ov = int(experiment.exp_dict['overSampling'])
    dimX = int(experiment.exp_dict['studyDimensions'][0])
    return (dimX // 2 - (ov - 1) / 2.0) / ov


def source_distance(experiment):
    """The distance from the source to the rotation axis in metres: distSourceToMembrane + distMembraneToObject, the
    denominator of the chain's magnification.  Needs no GPU."""
    ed = experiment.exp_dict
    return float(ed['distSourceToMembrane']) + float(ed['distMembraneToObject'])


def voxel_size(experiment):
    """The voxel of a scan's volume in metres: the detector pixel demagnified to the object, p/M."""
    return float(experiment.myDetector.det_param['myPixelSize']) * 1e-6 / float(experiment.exp_dict['magnification'])


def scan(experiment, angles_deg, modality='attenuation', differential=False, beam='parallel', **retrieve_options):
    """Run the chain of `experiment` (an Experiment, or the exp_dict of one) once per angle of angles_deg, all of its
    nbExpPoints membrane positions each time, and collect one map per angle and energy bin ->
    {'sinograms': {bin: [A, n, m] float32 tensor}, 'angles': the angles, 'center': rotation_center(experiment),
     'voxel_m': voxel_size(experiment), 'modality': modality, 'differential': differential,
     'energy_keV': the run's mean detected energy}.
    modality='attenuation': -ln(Propag/White) of position 0 (the propagation image over its flat field; any number of
    positions), for mu_volume.  modality='phase': 'phi' of retrieval.retrieve on the angle's positions (retrieve_options:
    method, max_shift, dark_field, window, search -- bound by retrieval.check_method's rules), for delta_volume.
    differential=True (modality 'phase' only, ValueError otherwise): the tracker runs without the integration
    (retrieval.retrieve(results, None, ...)) and the angle's map is dy * retrieval.gradient_scale(...), dy the displacement
    along map axis 1 = sinogram axis 2: d(phi)/d(column) in radians per detector pixel, what reconstruct then back-projects
    through the Hilbert filter.
    The sample of interest must be the contrast phantom or a label volume (ValueError otherwise): per angle its myAngle is
    set and its geometry rebuilt on the study grid.  A membrane that has a geometry function gets its geometry per position as main.run
    does; an injected one keeps the geometry it has.
    beam='cone': the sample (a label volume; the contrast phantom is refused, and so is differential=True) is projected
    from the experiment's point source, source_distance(experiment) from the rotation axis -- its mySourceDistance is set
    for the scan and restored --, the angles are meant to cover a full turn, and the result also holds 'beam',
    'source_px' (that distance in voxels of voxel_size) and 'row_center' (optical_row): what reconstruct's FDK needs.  A
    parallel scan's result has none of the three."""
    import torch
    from . import retrieval
    if modality not in MODALITIES:
        raise ValueError("modality must be one of %s, got %r" % (", ".join(MODALITIES), modality))
    check_differential(differential, modality, DEFAULT_METHOD)
    check_beam(beam, differential, DEFAULT_METHOD)
    if isinstance(experiment, dict):
        from .Experiment import Experiment
        experiment = Experiment(experiment)
    ed = experiment.exp_dict
    sample = _phantom(experiment.mySampleofInterest)
    npos = int(ed['nbExpPoints'])
    if modality == 'phase':
        retrieval.check_method(retrieve_options.get('method', 'lcs'), npos, retrieve_options.get('max_shift'),
                               retrieve_options.get('dark_field', False))
    elif retrieve_options:
        raise ValueError("%s are options of modality='phase'" % ", ".join(sorted(retrieve_options)))
    angles = list(_angles(angles_deg))
    sinos = {}
    cone = {}
    if beam == 'cone':
        cone = {'beam': beam, 'source_px': source_distance(experiment) / voxel_size(experiment),
                'row_center': optical_row(experiment)}
    with _diverging(sample, source_distance(experiment) if cone else None):
        _scan_angles(experiment, sample, angles, modality, differential, retrieve_options, sinos)
    return dict({'sinograms': {b: torch.stack(v) for b, v in sinos.items()}, 'angles': angles,
                 'center': rotation_center(experiment), 'voxel_m': voxel_size(experiment), 'modality': modality,
                 'differential': bool(differential), 'energy_keV': float(ed['meanEnergy'])}, **cone)


def _scan_angles(experiment, sample, angles, modality, differential, retrieve_options, sinos):
    """scan's loop: the chain at every angle, its maps appended to sinos[bin]."""
    import torch
    from . import retrieval
    ed = experiment.exp_dict
    npos = int(ed['nbExpPoints'])
    membrane = experiment.myMembrane
    for angle in angles:
        _turn(sample, angle, ed['studyDimensions'], ed['studyPixelSize'], ed['overSampling'])
        ed['meanEnergy'] = 0                       # every angle is a run of its own (the chain folds the positions' means into it)
        results = {}
        for pointNum in range(npos if modality == 'phase' else 1):
            if getattr(membrane, "myGeometryFunction", ""):
                membrane.myGeometry = []
                membrane.getMyGeometry(ed['studyDimensions'], membrane.membranePixelSize, ed['overSampling'], pointNum, npos)
            results[pointNum] = experiment.computeSampleAndReferenceImages(pointNum)
        experiment.resolve_mean_energy()
        if modality == 'attenuation':
            P, W = results[0][2], results[0][3]
            maps = {b: -torch.log(P[b] / W[b]) for b in range(P.shape[0])}
        else:
            params = retrieval.params_from_experiment(experiment)
            if differential:
                scale = retrieval.gradient_scale(**params)
                maps = {b: r['dy'] * scale for b, r in retrieval.retrieve(results, None, **retrieve_options).items()}
            else:
                maps = {b: r['phi'].clone() for b, r in retrieval.retrieve(results, params, **retrieve_options).items()}
        for b, v in maps.items():
            sinos.setdefault(b, []).append(v)


# The reconstruction methods, keyed by what the user says.  Each row: the solver, and whether the method takes (and then
# needs) iterations, takes (and needs) a weight, takes nonneg.  A new method is a new row.
Method = collections.namedtuple("Method", "solver iterations weight nonneg")
RECONSTRUCTIONS = {
    'fbp': Method(fbp, False, False, False),
    'sirt': Method(sirt, True, False, True),
    'cgls': Method(cgls, True, False, False),
    'tv': Method(tv, True, True, True),
}
METHODS = tuple(m for m, row in RECONSTRUCTIONS.items() if not row.weight)
REGULARISED_METHODS = tuple(m for m, row in RECONSTRUCTIONS.items() if row.weight)
DEFAULT_METHOD = 'fbp'
# what reconstruct's filter means for a differential scan: the same window on the Hilbert filter
DIFFERENTIAL_FILTER_OF = {'ramp': 'hilbert', 'hann': 'hilbert-hann'}


def check_reconstruction(method, iterations, nonneg=False, weight=None):
    """The rules of reconstruct's method options (ValueError): needs no GPU."""
    row = RECONSTRUCTIONS.get(method)
    if row is None:
        raise ValueError("method must be one of %s, got %r" % (", ".join(RECONSTRUCTIONS), method))
    if not row.iterations:
        if iterations is not None:
            raise ValueError("iterations is an option of the iterative methods (sirt, cgls), not of %s" % method)
    elif iterations is None:
        raise ValueError("method %r needs iterations" % method)
    else:
        _iterations(iterations)
    if row.weight:
        if weight is None:
            raise ValueError("method %r needs weight" % method)
        _weight(weight)
    elif weight is not None:
        raise ValueError("weight is an option of method 'tv'")
    if nonneg and not row.nonneg:
        raise ValueError("nonneg is an option of method 'sirt'")


def check_differential(differential, modality, method):
    """The differential route's rules (ValueError): a phase sinogram, reconstructed by filtered back-projection."""
    if differential and modality != 'phase':
        raise ValueError("differential is an option of modality 'phase', not of %r" % (modality,))
    if differential and method != 'fbp':
        raise ValueError("a differential sinogram is reconstructed by method 'fbp' (the Hilbert filter), not by %r: the "
                         "iterative methods solve B^T x = b for integral data" % (method,))


def check_beam(beam, differential, method):
    """The cone beam's rules (ValueError): an integral scan, reconstructed by method 'fbp', which is then FDK."""
    if beam not in BEAMS:
        raise ValueError("beam must be one of %s, got %r" % (", ".join(BEAMS), beam))
    if beam == 'cone' and differential:
        raise ValueError("a cone-beam scan has no differential form: the Hilbert-filter back-projection is parallel-beam")
    if beam == 'cone' and method != 'fbp':
        raise ValueError("method %r has no cone-beam form" % (method,))


def check_run_options(angles, modality, method, iterations, weight, differential=False, beam='parallel'):
    """The rules of main.run's tomography options (ValueError; needs no GPU): `angles` projections, 0 for no tomography;
    iterations 0 for none."""
    if modality not in MODALITIES:
        raise ValueError("tomography_modality must be one of %s, got %r" % (", ".join(MODALITIES), modality))
    if beam not in BEAMS:
        raise ValueError("tomography_beam must be one of %s, got %r" % (", ".join(BEAMS), beam))
    if beam != BEAMS[0] and not angles:
        raise ValueError("tomography_beam is an option of tomography")
    if differential and not angles:
        raise ValueError("tomography_differential is an option of tomography")
    check_differential(differential, modality, method)
    if modality != MODALITIES[0] and not angles:
        raise ValueError("tomography_modality is an option of tomography")
    if (method != DEFAULT_METHOD or iterations) and not angles:
        raise ValueError("tomography_method and tomography_iterations are options of tomography")
    if weight is not None and not angles:
        raise ValueError("tomography_weight is an option of tomography")
    check_reconstruction(method, iterations or None, weight=weight)
    check_beam(beam, differential, method)
    if int(angles) < 0 or int(angles) > _lib.PSX_FBP_MAX_ANGLES:
        raise ValueError("tomography takes 1 to %d angles, got %r" % (_lib.PSX_FBP_MAX_ANGLES, angles))


def add_tomography_options(ap):
    """--tomography and --tomography-modality, -differential, -method, -iterations, -weight, -beam on an argparse parser:
    main.py's."""
    iterative = "|".join(m for m, row in RECONSTRUCTIONS.items() if row.iterations)
    ap.add_argument("--tomography", type=int, default=0, metavar="A",
                    help="contrast-phantom and label-volume (getVolumeFromFile) samples: scan A angles (1..%d) on [0, 180) after "
                         "the run and write the filtered back-projection, tomography/{mu|delta}_<expID> under each bin's directory"
                    % _lib.PSX_FBP_MAX_ANGLES)
    ap.add_argument("--tomography-modality", default=MODALITIES[0], choices=MODALITIES,
                    help="--tomography: mu from -ln(Propag/White) (default), or delta from the retrieved phi (the rules and "
                         "options of --retrieve)")
    ap.add_argument("--tomography-differential", action="store_true",
                    help="--tomography-modality phase with --tomography-method fbp: back-project the tracked gradient across "
                         "the rotation axis through a Hilbert filter; no phase integration is run")
    ap.add_argument("--tomography-method", default=DEFAULT_METHOD, choices=tuple(RECONSTRUCTIONS),
                    help="--tomography: filtered back-projection (default), or --tomography-iterations steps of SIRT, CGLS or "
                         "total-variation reconstruction (tv, with --tomography-weight)")
    ap.add_argument("--tomography-iterations", type=int, default=0, metavar="K",
                    help="--tomography-method %s: the number of iterations (>= 1)" % iterative)
    ap.add_argument("--tomography-weight", type=float, default=None, metavar="W",
                    help="--tomography-method %s: the weight of the total variation, relative to the sinogram's largest "
                         "value (>= 0)" % "|".join(REGULARISED_METHODS))
    ap.add_argument("--tomography-beam", default=BEAMS[0], choices=BEAMS,
                    help="--tomography: parallel rays (default), or cone: a label-volume sample is projected from the experiment's "
                         "point source, the A angles lie on [0, 360) and --tomography-method fbp reconstructs by FDK")


def check_tomography_options(ap, a):
    """The rules of add_tomography_options' seven, as ap.error: all are options of --tomography, and which of them the
    method and the beam take."""
    if a.tomography < 0:
        ap.error("--tomography takes a number of angles >= 1")
    for option, given in (("modality", a.tomography_modality != MODALITIES[0]), ("method", a.tomography_method != DEFAULT_METHOD),
                          ("iterations", a.tomography_iterations != 0), ("weight", a.tomography_weight is not None),
                          ("differential", a.tomography_differential), ("beam", a.tomography_beam != BEAMS[0])):
        if given and not a.tomography:
            ap.error("--tomography-%s is an option of --tomography" % option)
    if a.tomography_differential and (a.tomography_modality != 'phase' or a.tomography_method != DEFAULT_METHOD):
        ap.error("--tomography-differential goes with --tomography-modality phase and --tomography-method fbp, and only with them")
    if a.tomography_beam == 'cone' and (a.tomography_differential or a.tomography_method != DEFAULT_METHOD):
        ap.error("--tomography-beam cone goes with --tomography-method fbp (FDK) and without --tomography-differential")
    row = RECONSTRUCTIONS[a.tomography_method]
    if row.weight != (a.tomography_weight is not None):
        ap.error("--tomography-weight W >= 0 goes with --tomography-method tv, and only with it")
    if a.tomography_weight is not None and not (0 <= a.tomography_weight < float("inf")):
        ap.error("--tomography-weight takes a finite weight >= 0")
    if row.weight and a.tomography_iterations < 1:
        ap.error("--tomography-method %s needs --tomography-iterations K >= 1" % a.tomography_method)
    if a.tomography_iterations < 0 or row.iterations != (a.tomography_iterations != 0):
        ap.error("--tomography-iterations K >= 1 goes with --tomography-method sirt or cgls, and only with them")


def reconstruct(scanned, filter='ramp', circle=True, method='fbp', iterations=None, nonneg=False, weight=None):
    """A scan's volumes in physical units -> {bin: [n, m, m] float32 tensor}: mu (1/m) for modality 'attenuation', delta for
    'phase' (at the scan's mean detected energy: right for one bin only, as retrieval.retrieve's default).  method: 'fbp'
    (with `filter`), or 'sirt' / 'cgls' with `iterations` steps from zero (required for them, refused for 'fbp'; `filter`
    is not used), or 'tv' with `iterations` steps and `weight` (both required, weight refused for the others); nonneg: the
    clamp of sirt and tv.  weight is RELATIVE: tv runs with weight * max|sinogram| per bin, so that scaling a sinogram
    scales its volume and one weight serves -ln T and radians alike.
    A differential scan (scanned['differential'], scan(..., differential=True); a dict without the key is an integral one)
    holds d(phi)/d(column) and goes through the Hilbert filter: filter 'ramp' then means 'hilbert' and 'hann' means
    'hilbert-hann', 'none' is refused, and so is every method but 'fbp' (ValueError): sirt, cgls and tv solve B^T x = b for
    integral data, and an iterative solver on the differentiated operator is out of scope here.  The conversion by
    delta_volume is the same.
    A cone-beam scan (scanned['beam'] == 'cone', scan(..., beam='cone'); a dict without the key is a parallel one) is
    reconstructed by FDK -- that is what method 'fbp' means for it -- with the scan's 'source_px' and 'row_center'; every
    other method is refused (ValueError)."""
    check_reconstruction(method, iterations, nonneg, weight)
    cone = scanned.get('beam', BEAMS[0]) == 'cone'
    check_beam(scanned.get('beam', BEAMS[0]), scanned.get('differential', False), method)
    if scanned.get('differential', False):
        check_differential(True, scanned['modality'], method)
        if filter not in DIFFERENTIAL_FILTER_OF:
            raise ValueError("a differential sinogram takes filter %s, got %r" % (" or ".join(DIFFERENTIAL_FILTER_OF), filter))
        filter = DIFFERENTIAL_FILTER_OF[filter]
    row = RECONSTRUCTIONS[method]
    options = {'iterations': iterations} if row.iterations else {'filter': filter}
    if row.nonneg:
        options['nonneg'] = nonneg
    out = {}
    for b, s in scanned['sinograms'].items():
        if row.weight:
            options['weight'] = float(weight) * float(s.abs().max())
        if cone:
            vol = fdk(s, scanned['angles'], scanned['source_px'], center=scanned['center'], row_center=scanned['row_center'],
                      circle=circle, **options)
        else:
            vol = row.solver(s, scanned['angles'], center=scanned['center'], circle=circle, **options)
        out[b] = (mu_volume(vol, scanned['voxel_m']) if scanned['modality'] == 'attenuation'
                  else delta_volume(vol, scanned['energy_keV'], scanned['voxel_m']))
    return out


def volume_name(modality):
    return "mu" if modality == 'attenuation' else "delta"


def save_volume(vol, path, fmt=".npy"):
    """Write an [n, m, m] volume (tensor or array): fmt '.npy' -> the one file path + '.npy' (float32 [n, m, m]); '.tif' /
    '.edf' -> the directory `path` with one image per slice, slice_<rrrr><fmt>.  -> the paths written."""
    from .InputOutput.pagailleIO import save_image
    v = np.ascontiguousarray(vol.detach().cpu().numpy() if hasattr(vol, "detach") else np.asarray(vol), dtype=np.float32)
    if v.ndim != 3:
        raise ValueError("a volume is [n, m, m], got shape %s" % (v.shape,))
    if fmt == ".npy":
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        np.save(path + fmt, v)
        return [path + fmt]
    os.makedirs(path, exist_ok=True)
    paths = []
    for r in range(v.shape[0]):
        paths.append(os.path.join(path, "slice_%04d%s" % (r, fmt)))
        save_image(v[r], paths[-1])
    return paths

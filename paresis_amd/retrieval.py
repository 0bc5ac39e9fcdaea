"""Speckle-tracking phase retrieval of the simulated image stacks, on the GPU.

A speckle-based run gives, per energy bin, K membrane positions of a sample image S_k and a reference image R_k.  This
module turns them into the sample's transmission, its refraction (displacement) and its phase:

    lcs(sample, reference)   LCS ("Low Coherence System", Quenot et al., Optica 8, 1412, 2021): per pixel, the float64
                             least-squares solution of  R_k ~ x0*S_k + x1*dR_k/d0 + x2*dR_k/d1  over the K positions,
                             the first-order form of S(r) = T*R(r - D): transmission = 1/x0, (dx, dy) = (x1, x2) in
                             detector pixels, along axis 0 / axis 1, with the sign of the chain's Dxreal / Dyreal;
                             dark_field=True (LCS-DF, K >= 4) adds the column x3*lap(R_k), the diffusion term of the X-ray
                             Fokker-Planck model (Morgan & Paganin, Sci. Rep. 9, 17465, 2019): df = -x3 in detector px^2
    umpa(sample, reference)  UMPA ("Unified Modulated Pattern Analysis", Zdora et al., PRL 118, 203903, 2017; separable form:
                             De Marco et al., Opt. Express 31, 635, 2023): per pixel, the integer shift |a|, |b| <= search
                             that minimises the float64 least-squares cost of S(q) = T*R(q - u) over a uniform
                             (2*window+1)^2 window (no Hamming taper, unlike the UMPA package) and the K >= 1 positions,
                             refined to sub-pixel by a parabola per axis: displacements of several pixels, where the
                             first-order LCS (|D| < 1 px) fails; also 'residual', the cost at the minimum over sum S^2;
                             dark_field=True fits S(q) = T*[mu + V*(R(q - u) - mu)], mu the reference frame's mean, and
                             adds 'visibility' V, UMPA's dark-field signal (1: no scattering)
    scattering_angle(df, ...) df -> the chain's scattering angle theta in radians
    phase_gradient(...)      displacement -> phase gradient in radians per detector pixel
    integrate(gx, gy)        Frankot-Chellappa (IEEE PAMI 10, 1988) with mirror extension -> phase (zero mean)
    retrieve(results, ...)   all of it for every bin of main.run's {position: (Sample, Reference, ...)}
    paganin(image, white)    propagation-based imaging's answer from the same run: Paganin's single-distance, single-material
                             filter (Paganin et al., J. Microsc. 206, 33, 2002) of the propagation image (the sample
                             without the membrane) over the flat field -> contact image, thickness and phase
    retrieve_propagation(results, ...)   paganin for every bin of main.run's position 0 (its Propag and White stacks)

All steps are HIP kernels (csrc/retrieve.hip, csrc/umpa.hip; the integration's transforms are rocFFT); nothing runs on the host but
argument checks.  Command line, for a run already on disk (main.py's layout):

    python -m paresis_amd.retrieval RUN_DIR [--energy KEV --pixel-um P --distance Z --magnification M]
                                            [--max-shift S] [--format .tif] [--dark-field]
                                            [--method {lcs,umpa,umpa-df} --window W --search M]

writes retrieval/{transmission,dx,dy,phi}_<expID><fmt> under each bin's directory; without the four physical parameters
only transmission, dx and dy.  --dark-field (4 positions or more) adds df, and scattering with the physical parameters.
--method umpa (1 position or more; no --dark-field, no --max-shift) tracks with UMPA and adds residual; --method umpa-df
(the same rules) also fits UMPA's dark-field term and adds visibility.

    python -m paresis_amd.retrieval RUN_DIR --propagation --delta D --beta B --energy KEV --pixel-um P --distance Z
                                            --magnification M [--format .tif]

writes propag/retrieval/{contact,thickness,phi}_<expID><fmt> under each bin's directory from its propag/PropagImage_ and
White_ pair (paganin; delta, beta: the sample's single material at --energy).  It takes none of the tracker options.
"""
import argparse
import collections
import os
import re
import sys

import numpy as np

from . import _lib
from .getk import getk

_plans = {}


# The trackers, keyed by what the user says: (method, dark_field).  Each row: the ops function, the fewest positions, the
# output maps in that function's order, and the options the method takes.  A new tracker is a new row.
Tracker = collections.namedtuple("Tracker", "op min_positions maps options")
TRACKERS = {
    ('lcs', False): Tracker('lcs', 3, ('transmission', 'dx', 'dy'), ('max_shift',)),
    ('lcs', True): Tracker('lcs_df', 4, ('transmission', 'dx', 'dy', 'df'), ('max_shift',)),
    ('umpa', False): Tracker('umpa', 1, ('transmission', 'dx', 'dy', 'residual'), ('window', 'search')),
    ('umpa-df', False): Tracker('umpa_df', 1, ('transmission', 'dx', 'dy', 'visibility', 'residual'), ('window', 'search', 'mean')),
}
METHODS = tuple(dict.fromkeys(m for m, _ in TRACKERS))
UMPA_METHODS = tuple(m for (m, _), t in TRACKERS.items() if 'window' in t.options)
# why a method of UMPA_METHODS has no row with dark_field=True
_NO_DARK_FIELD = {'umpa': "has no dark-field term", 'umpa-df': "always fits its dark-field term"}
# every map a bin's result may hold, in the order save_retrieval writes them
MAP_ORDER = ("transmission", "dx", "dy", "phi", "df", "scattering", "visibility", "residual")
assert all(set(t.maps) <= set(MAP_ORDER) for t in TRACKERS.values())


def _track(key, sample, reference, **options):
    """One bin through the tracker of TRACKERS[key] -> {map name: n x m float32 tensor}."""
    from . import ops
    t = TRACKERS[key]
    return dict(zip(t.maps, getattr(ops, t.op)(sample, reference, **options)))


def lcs(sample, reference, max_shift=None, dark_field=False):
    """K >= 3 sample / reference images of one bin ([K, n, m] float32 CUDA tensors, or sequences of K n x m ones) ->
    {'transmission', 'dx', 'dy'}, n x m float32 on the same device.  max_shift (pixels): clamp dx, dy; None: no clamp.
    dark_field: LCS-DF (K >= 4, ops.lcs_df) -- the four-unknown system, whose transmission and displacement are not biased
    by the lost speckle visibility of a scattering sample, and 'df' (detector px^2, unclamped) in the dict."""
    return _track(('lcs', bool(dark_field)), sample, reference, max_shift=max_shift)


def umpa(sample, reference, window=2, search=3, dark_field=False, mean=None):
    """K >= 1 sample / reference images of one bin (the forms lcs takes) -> {'transmission', 'dx', 'dy', 'residual'}, n x m
    float32 on the same device (ops.umpa): the shift of a uniform (2*window+1)^2 window within |a|, |b| <= search pixels,
    sub-pixel by a parabola per axis.  Pixels closer than window+search to a border are (1, 0, 0, 0).
    dark_field: the three-modality model S = T*[mu + V*(R(q - u) - mu)] (ops.umpa_df), and 'visibility' V in the dict: the
    speckle visibility behind the sample over the reference's, 1 in the border band, not clamped.  mean: the K reference
    means mu_k (None: computed on the device, which synchronises).  V is not converted to a scattering angle: that
    conversion depends on the speckle's spectrum."""
    key = ('umpa-df' if dark_field else 'umpa', False)
    options = {'window': window, 'search': search}
    if 'mean' in TRACKERS[key].options:
        options['mean'] = mean
    elif mean is not None:
        raise ValueError("mean is an option of dark_field=True")
    return _track(key, sample, reference, **options)


def check_method(method, npos, max_shift=None, dark_field=False):
    """The argument rules of retrieve(): ValueError for an unknown method, too few positions (lcs: 3, LCS-DF: 4, umpa and
    umpa-df: 1), or umpa / umpa-df with dark_field or max_shift.  Needs no GPU.  -> the method's key in TRACKERS."""
    if method not in METHODS:
        raise ValueError("method must be one of %s, got %r" % (", ".join(METHODS), method))
    key = (method, bool(dark_field))
    if key not in TRACKERS:
        raise ValueError("method=%r %s: dark_field is an option of method='lcs'" % (method, _NO_DARK_FIELD[method]))
    if max_shift is not None and 'max_shift' not in TRACKERS[key].options:
        raise ValueError("method=%r is bounded by its search range: max_shift is an option of method='lcs'" % method)
    least = TRACKERS[(method, False)].min_positions
    if npos < least:
        raise ValueError("phase retrieval needs at least %d position%s, got %d" % (least, "s" if least > 1 else "", npos))
    if npos < TRACKERS[key].min_positions:
        raise ValueError("dark-field retrieval needs at least %d positions, got %d" % (TRACKERS[key].min_positions, npos))
    return key


def _plan(device, n, m):
    import torch
    from . import ops
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), int(n), int(m))
    p = _plans.get(key)
    if p is None:
        p = _plans[key] = ops.IntegratePlan(n, m, device=torch.device("cuda", key[0]))
    return p


def integrate(gx, gy, scale=1.0, out=None):
    """Frankot-Chellappa integration of the gradient field scale*(gx, gy) (n x m float32 CUDA tensors, radians per pixel along
    axis 0 / axis 1) with mirror extension -> phi, n x m float32, zero mean over the 2n x 2m extension.  One plan per
    (device, shape) is kept for the process's lifetime."""
    return _plan(gx.device, gx.shape[0], gx.shape[1]).integrate(gx, gy, scale=scale, out=out)


def gradient_scale(energy_keV, pixel_um, distance_m, magnification):
    """Radians per detector pixel of phase gradient per detector pixel of displacement: k*p^2/(M*z).

    The ray-tracing chain displaces by D = dphi/di * z/(k*h^2*M) study pixels (refractionFileNumba2.py:54-56, gradient per
    study pixel of size h = p/(ov*M), M the object->detector magnification the chain passes, EXP:473-474), and the detector
    bins ov x ov study pixels into one.  A phase slope s per detector pixel is s/ov per study pixel, so
    D = (s/ov)*z/(k*h^2*M) study pixels = (s/ov^2)*z/(k*h^2*M) detector pixels = s*z*M/(k*p^2), i.e. s = D*k*p^2/(M*z);
    ov drops out.  k = getk(E), the chain's own constants."""
    p = float(pixel_um) * 1e-6
    return getk(float(energy_keV) * 1e3) * p * p / (float(magnification) * float(distance_m))


def scattering_angle(df, pixel_um, distance_m):
    """The chain's scattering angle theta (radians) from LCS-DF's df (detector px^2): theta = 2*p*sqrt(2*max(df, 0))/z.

    The ray-tracing chain turns theta into a Gaussian re-splat of sigma = theta*z/(h*M)/2 study pixels
    (refractionFileNumba2.py:114, gaussian_shape(DF/2)), h = p/(ov*M) the study pixel (Experiment.py:188), M the
    object->detector magnification the chain passes, so sigma_study = theta*z*ov/(2*p).  The detector bins ov x ov study
    pixels into one: sigma_det = sigma_study/ov = theta*z/(2*p) detector pixels.  A Gaussian blur of per-axis variance s^2 is
    to first order f + (s^2/2)*lap f, so df = sigma_det^2/2, i.e. theta = 2*p*sqrt(2*df)/z; ov, M and the energy drop out.
    Negative df (noise, model error) gives 0.  df: a tensor or a numpy array; pixel_um: the detector pixel; distance_m:
    distObjectToDetector."""
    c = 2.0 * float(pixel_um) * 1e-6 / float(distance_m)
    if hasattr(df, "clamp"):
        return c * (2.0 * df.clamp(min=0)).sqrt()
    return c * np.sqrt(2.0 * np.maximum(df, 0))


def phase_gradient(dx, dy, energy_keV, pixel_um, distance_m, magnification):
    """(gx, gy) = (dx, dy) * k*p^2/(M*z): displacements in detector pixels -> phase gradient in radians per detector pixel
    (see gradient_scale).  energy_keV: the photon energy; pixel_um: the detector pixel; distance_m: distObjectToDetector;
    magnification: exp_dict['magnification'].  Tensors or numpy arrays."""
    c = gradient_scale(energy_keV, pixel_um, distance_m, magnification)
    return dx * c, dy * c


def paganin_alpha(delta, beta, energy_keV, pixel_um, distance_m, magnification):
    """(alpha, mu) of Paganin's filter 1/(1 + alpha*k^2), k in radians per detector pixel: mu = 2*k0*beta (1/m) and
    alpha = z*M*delta/(mu*p^2) (detector px^2).  Needs no GPU.

    A single material of thickness t attenuates by exp(-mu*t), mu = 2*k0*beta, and shifts the phase by phi = -k0*delta*t,
    k0 = getk(E) (the chain's constants; Sample.setWave's -k*delta*t and -k*beta*t on the amplitude).  Propagating the wave
    over an effective distance d on a grid of spacing h, the transport-of-intensity equation gives, for that material,
    I/I0 = (1 - (d*delta/mu)*lap) exp(-mu*t), lap the Laplacian in metres: in pixels of size h the operator is
    1 + alpha_h*k^2 with alpha_h = d*delta/(mu*h^2).  The chain propagates the cone beam as a parallel one over d = z/M
    on the study grid h = p/(ov*M) (z = distObjectToDetector, M the object->detector magnification it passes, p the
    detector pixel, ov the oversampling), so alpha_h = (z/M)*delta*ov^2*M^2/(mu*p^2) study px^2; the detector bins ov x ov
    study pixels into one, and a frequency per detector pixel is ov times the frequency per study pixel, so
    alpha = alpha_h/ov^2 = z*M*delta/(mu*p^2) detector px^2; ov drops out, as in gradient_scale.  delta, beta: the
    material's index decrements at energy_keV; pixel_um: the detector pixel; distance_m: distObjectToDetector;
    magnification: exp_dict['magnification']."""
    delta, beta = float(delta), float(beta)
    p = float(pixel_um) * 1e-6
    z, M = float(distance_m), float(magnification)
    if not (delta >= 0.0 and np.isfinite(delta)):
        raise ValueError("delta must be finite and >= 0, got %r" % delta)
    if not (beta > 0.0 and np.isfinite(beta)):
        raise ValueError("beta must be finite and > 0 (a material that does not absorb has no Paganin filter), got %r" % beta)
    if not (float(energy_keV) > 0.0 and p > 0.0 and z >= 0.0 and M > 0.0):
        raise ValueError("energy_keV, pixel_um and magnification must be > 0 and distance_m >= 0")
    mu = 2.0 * getk(float(energy_keV) * 1e3) * beta
    return z * M * delta / (mu * p * p), mu


def _per_image(v, B):
    return [float(v)] * B if np.ndim(v) == 0 else [float(x) for x in v]


def paganin(image, white=None, *, delta, beta, energy_keV, pixel_um, distance_m, magnification):
    """Paganin's single-distance, single-material retrieval of a propagation image (ops.paganin, psx_paganin_f32; the
    filter's units: paganin_alpha) -> {'contact', 'thickness', 'phi'}, float32 on the image's device:
    contact = exp(-mu*t) as it would be measured at the sample (I/I0 with the propagation fringes filtered out),
    thickness = t of the material in metres, phi = -k*delta*t in radians (k = getk(E), Sample.setWave's phase).
    image: one n x m float32 CUDA tensor -> n x m maps; or a [B, n, m] stack / a sequence of B images -> [B, n, m] maps,
    with delta, beta and energy_keV one number each or B of them (the bins of a run differ in energy).  white: the flat
    field(s) in the same form, None when the image is already I/I0.  The plan is retrieval's own per (device, shape):
    a shape shared with integrate() uses one buffer."""
    import torch
    from . import ops
    single = isinstance(image, torch.Tensor) and image.dim() == 2
    images = [image] if single else image
    whites = [white] if single and white is not None else white
    I = ops._image_list(images, "image")
    B = len(I)
    try:
        d, b, e = _per_image(delta, B), _per_image(beta, B), _per_image(energy_keV, B)
    except (TypeError, ValueError):
        raise ValueError("delta, beta and energy_keV must be numbers or sequences of %d numbers" % B)
    if not len(d) == len(b) == len(e) == B:
        raise ValueError("delta, beta and energy_keV must hold one value per image (%d), got %d, %d, %d" % (B, len(d), len(b), len(e)))
    am = [paganin_alpha(d[i], b[i], e[i], pixel_um, distance_m, magnification) for i in range(B)]
    for i, t in enumerate(I):
        ops._need(t, torch.float32, "image[%d]" % i)          # before a plan is looked up on the image's device
    n, m = I[0].shape
    contact, thickness = ops.paganin(I, whites, [a for a, _ in am], [u for _, u in am], _plan(I[0].device, n, m))
    c = torch.tensor([-getk(e[i] * 1e3) * d[i] for i in range(B)], dtype=torch.float32, device=thickness.device)
    r = {'contact': contact, 'thickness': thickness, 'phi': thickness * c[:, None, None]}
    return {k: v[0] for k, v in r.items()} if single else r


PROPAGATION_MAPS = ("contact", "thickness", "phi")


def propagation_material(experiment, material=None):
    """The single material Paganin's filter assumes, of an Experiment: by default the sample of interest's first one;
    a name that is not among the sample's materials is a ValueError.  Needs no GPU."""
    mats = list(experiment.mySampleofInterest.myMaterials)
    if material is None:
        if not mats:
            raise ValueError("the sample of interest names no material")
        return mats[0]
    if material not in mats:
        raise ValueError("material %r is not one of the sample of interest's (%s)" % (material, ", ".join(map(str, mats))))
    return material


def retrieve_propagation(results, params, delta_beta, bins=None, energies=None, device=None):
    """Paganin retrieval of every bin of a run's propagation image: results = main.run's {position: (Sample, Reference, Propag,
    White, ...)}, of which position 0's [nbins, n, m] Propag and White stacks are read (host or device; host stacks are
    uploaded once) -> {bin: {'contact', 'thickness', 'phi'}}, device tensors.  params: params_from_experiment's dict.
    delta_beta: (delta, beta) of the sample's single material, or the material's name, resolved at each bin's energy
    through materials.delta_beta.  bins, energies: as retrieve() -- without energies every bin uses params['energy_keV'],
    which is right for one bin only.  All bins go through one ops.paganin call per PSX_MAX_PAGANIN of them."""
    if 0 not in results or len(results[0]) < 4:
        raise ValueError("results hold no propagation image: position 0's (Sample, Reference, Propag, White) is needed")
    import torch
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    P = _stack(results, [0], 2, dev)[0]
    W = _stack(results, [0], 3, dev)[0]
    bins = list(range(P.shape[0])) if bins is None else [int(b) for b in bins]
    if energies is not None and len(energies) != len(bins):
        raise ValueError("energies must hold one value per retrieved bin (%d), got %d" % (len(bins), len(energies)))
    e = [float(params['energy_keV'])] * len(bins) if energies is None else [float(v) for v in energies]
    if isinstance(delta_beta, str):
        from . import materials
        db = [materials.delta_beta(delta_beta, v) for v in e]
    else:
        db = [(float(delta_beta[0]), float(delta_beta[1]))] * len(bins)
    out = {}
    for i0 in range(0, len(bins), _lib.PSX_MAX_PAGANIN):
        sl = slice(i0, i0 + _lib.PSX_MAX_PAGANIN)
        r = paganin([P[b] for b in bins[sl]], [W[b] for b in bins[sl]], delta=[d for d, _ in db[sl]], beta=[b for _, b in db[sl]],
                    energy_keV=e[sl], pixel_um=params['pixel_um'], distance_m=params['distance_m'],
                    magnification=params['magnification'])
        for i, b in enumerate(bins[sl]):
            out[b] = {k: r[k][i] for k in PROPAGATION_MAPS}
    return out


def save_propagation(r, directory, exp_id, fmt):
    """Write one bin's Paganin maps as directory/propag/retrieval/<name>_<exp_id><fmt> (name: contact, thickness, phi)."""
    from .InputOutput.pagailleIO import save_image
    d = os.path.join(directory, "propag", "retrieval")
    os.makedirs(d, exist_ok=True)
    paths = []
    for name in PROPAGATION_MAPS:
        paths.append(os.path.join(d, "%s_%s%s" % (name, exp_id, fmt)))
        save_image(r[name].detach().cpu().numpy(), paths[-1])
    return paths


def params_from_experiment(experiment):
    """The physical parameters of an Experiment's retrieval: {'energy_keV': exp_dict['meanEnergy'] (known after a run),
    'pixel_um': the detector pixel, 'distance_m': distObjectToDetector, 'magnification': exp_dict['magnification']}."""
    ed = experiment.exp_dict
    return {'energy_keV': float(ed['meanEnergy']), 'pixel_um': float(experiment.myDetector.det_param['myPixelSize']),
            'distance_m': float(ed['distObjectToDetector']), 'magnification': float(ed['magnification'])}


def _stack(results, positions, slot, device):
    import torch
    imgs = [results[p][slot] for p in positions]
    if all(isinstance(t, torch.Tensor) and t.is_cuda for t in imgs):
        return [t.to(device=device, dtype=torch.float32).contiguous() for t in imgs]
    host = np.stack([np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32) for t in imgs])
    dev = torch.from_numpy(host).to(device)                         # one upload: [K, nbins, n, m]
    return [dev[k] for k in range(dev.shape[0])]


def retrieve(results, params=None, bins=None, energies=None, max_shift=None, device=None, dark_field=False, method='lcs',
             window=2, search=3):
    """Retrieve every bin of a run: results = main.run's {position: (Sample, Reference, ...)} with [nbins, n, m] stacks (host or
    device; host stacks are uploaded once) -> {bin: {'transmission', 'dx', 'dy', 'phi'}}, device tensors.

    params: {'energy_keV', 'pixel_um', 'distance_m', 'magnification'} (params_from_experiment); None: no phase ('phi' left
    out).  bins: the bins to retrieve (default all).  energies: one energy (keV) per bin of `bins`; without it every bin uses
    params['energy_keV'] -- the run's mean detected energy, which is right for one bin only: a multi-bin run should pass
    each bin's own energy.  max_shift: clamp of dx, dy in pixels (None: no clamp).  dark_field: LCS-DF (4 positions or
    more): every bin also gets 'df' (detector px^2) and, with params, 'scattering' (theta, radians; scattering_angle);
    'phi' then integrates the four-unknown system's dx, dy.  method='umpa' (1 position or more; window, search: umpa's):
    every bin's maps come from umpa() instead, with 'residual'; 'phi' integrates its dx, dy the same way.  It takes neither
    dark_field nor max_shift (ValueError).  method='umpa-df': umpa(dark_field=True), the same rules; every bin gains
    'visibility' as well (no scattering angle is derived from it)."""
    positions = sorted(results)
    key = check_method(method, len(positions), max_shift, dark_field)
    options = {'max_shift': max_shift, 'window': window, 'search': search}
    options = {k: v for k, v in options.items() if k in TRACKERS[key].options}
    import torch
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    S = _stack(results, positions, 0, dev)
    R = _stack(results, positions, 1, dev)
    nbins = S[0].shape[0]
    bins = list(range(nbins)) if bins is None else [int(b) for b in bins]
    if energies is not None and len(energies) != len(bins):
        raise ValueError("energies must hold one value per retrieved bin (%d), got %d" % (len(bins), len(energies)))
    out = {}
    for i, b in enumerate(bins):
        r = _track(key, [s[b] for s in S], [s[b] for s in R], **options)
        if params is not None:
            e = params['energy_keV'] if energies is None else energies[i]
            r['phi'] = integrate(r['dx'], r['dy'],
                                 scale=gradient_scale(e, params['pixel_um'], params['distance_m'], params['magnification']))
            if 'df' in r:
                r['scattering'] = scattering_angle(r['df'], params['pixel_um'], params['distance_m'])
        out[b] = r
    return out


def save_retrieval(r, directory, exp_id, fmt):
    """Write one bin's maps as directory/retrieval/<name>_<exp_id><fmt> (name: transmission, dx, dy[, phi][, df][, scattering]
    [, visibility][, residual])."""
    from .InputOutput.pagailleIO import save_image
    d = os.path.join(directory, "retrieval")
    os.makedirs(d, exist_ok=True)
    paths = []
    for name in MAP_ORDER:
        if name in r:
            paths.append(os.path.join(d, "%s_%s%s" % (name, exp_id, fmt)))
            save_image(r[name].detach().cpu().numpy(), paths[-1])
    return paths


_SAMPLE = re.compile(r"^sampleImage_(.+)_(\d+)(\.[A-Za-z0-9]+)$")
_REF = re.compile(r"^ReferenceImage_(.+)_(\d+)(\.[A-Za-z0-9]+)$")


def discover(run_dir, min_positions=3):
    """main.run's layout under run_dir -> [(bin_dir, exp_id, fmt, [(position, sample_path, reference_path), ...])], one entry
    per bin directory (run_dir itself for a one-bin run, run_dir/NN_NNkev/ otherwise), positions in increasing order.
    Raises ValueError when a sample has no reference partner (or the reverse), when one directory holds several runs or
    formats, or when fewer than min_positions positions are found (3: LCS; UMPA takes 1).  Needs no GPU."""
    run_dir = os.path.abspath(run_dir)
    cands = [run_dir] + sorted(os.path.join(run_dir, d) for d in os.listdir(run_dir)
                               if re.match(r"^\d+_\d+kev$", d) and os.path.isdir(os.path.join(run_dir, d)))
    found = []
    for d in cands:
        sd, rd = os.path.join(d, "sample"), os.path.join(d, "ref")
        if not os.path.isdir(sd) and not os.path.isdir(rd):
            continue
        side = []
        for sub, pat in ((sd, _SAMPLE), (rd, _REF)):
            files = {}
            for f in sorted(os.listdir(sub)) if os.path.isdir(sub) else []:
                mt = pat.match(f)
                if mt:
                    files[(mt.group(1), int(mt.group(2)), mt.group(3))] = os.path.join(sub, f)
            side.append(files)
        s, r = side
        for key in sorted(set(s) ^ set(r)):
            raise ValueError("%s: %s image of run %s position %d (%s) has no %s partner"
                             % (d, "sample" if key in s else "reference", key[0], key[1], key[2],
                                "reference" if key in s else "sample"))
        runs = sorted({(k[0], k[2]) for k in s})
        if not runs:
            continue
        if len(runs) > 1:
            raise ValueError("%s holds several runs or formats %s: give one run's directory" % (d, runs))
        exp_id, fmt = runs[0]
        pos = sorted(k[1] for k in s)
        if len(pos) < min_positions:
            raise ValueError("%s: phase retrieval needs at least %d positions, found %d" % (d, min_positions, len(pos)))
        found.append((d, exp_id, fmt, [(p, s[(exp_id, p, fmt)], r[(exp_id, p, fmt)]) for p in pos]))
    if not found:
        raise ValueError("no sample/ and ref/ images of main.run's layout under %s" % run_dir)
    return found


_PROPAG = re.compile(r"^PropagImage_(.+)_(\.[A-Za-z0-9]+)$")
_WHITE = re.compile(r"^White_(.+)_(\.[A-Za-z0-9]+)$")


def discover_propagation(run_dir):
    """main.run's layout under run_dir -> [(bin_dir, exp_id, fmt, propag_path, white_path)], one entry per bin directory
    (discover's candidates) that holds propag/PropagImage_<id>_<fmt> and White_<id>_<fmt>.  Raises ValueError when a
    propagation image has no flat field (or the reverse), when one directory holds several runs or formats, or when
    nothing is found.  Needs no GPU."""
    run_dir = os.path.abspath(run_dir)
    cands = [run_dir] + sorted(os.path.join(run_dir, d) for d in os.listdir(run_dir)
                               if re.match(r"^\d+_\d+kev$", d) and os.path.isdir(os.path.join(run_dir, d)))
    found = []
    for d in cands:
        side = []
        for sub, pat in ((os.path.join(d, "propag"), _PROPAG), (d, _WHITE)):
            files = {}
            for f in sorted(os.listdir(sub)) if os.path.isdir(sub) else []:
                mt = pat.match(f)
                if mt and os.path.isfile(os.path.join(sub, f)):
                    files[(mt.group(1), mt.group(2))] = os.path.join(sub, f)
            side.append(files)
        pg, wh = side
        for key in sorted(set(pg) ^ set(wh)):
            raise ValueError("%s: %s of run %s (%s) has no %s partner"
                             % (d, "propagation image" if key in pg else "flat field", key[0], key[1],
                                "flat field (White_)" if key in pg else "propagation image (propag/PropagImage_)"))
        if not pg:
            continue
        if len(pg) > 1:
            raise ValueError("%s holds several runs or formats %s: give one run's directory" % (d, sorted(pg)))
        (exp_id, fmt), = pg
        found.append((d, exp_id, fmt, pg[(exp_id, fmt)], wh[(exp_id, fmt)]))
    if not found:
        raise ValueError("no propag/PropagImage_ and White_ images of main.run's layout under %s" % run_dir)
    return found


def retrieve_propagation_run_dir(run_dir, params, delta, beta, fmt=None):
    """discover_propagation() + paganin + save_propagation for every bin directory; returns the paths.  params:
    params_from_experiment's four; delta, beta: the sample's material at params['energy_keV']."""
    import torch
    from .InputOutput.pagailleIO import openImage
    found = discover_propagation(run_dir)                          # before the device: a wrong directory needs no GPU
    written = []
    dev = torch.device("cuda", torch.cuda.current_device())
    for d, exp_id, in_fmt, pg, wh in found:
        P = torch.from_numpy(np.asarray(openImage(pg), dtype=np.float32)[None]).to(dev)
        W = torch.from_numpy(np.asarray(openImage(wh), dtype=np.float32)[None]).to(dev)
        res = retrieve_propagation({0: (None, None, P, W)}, params, (delta, beta))[0]
        written += save_propagation(res, d, exp_id, fmt or in_fmt)
    return written


def _first_floor(method):
    """The fewest positions discover() asks for: the method's without dark field (an unknown method is retrieve()'s to report,
    after discovery as ever: LCS's floor)."""
    return TRACKERS.get((method, False), TRACKERS[('lcs', False)]).min_positions


def _retrieve_found(found, params, fmt, **how):
    import torch
    from .InputOutput.pagailleIO import openImage
    written = []
    dev = torch.device("cuda", torch.cuda.current_device())
    for d, exp_id, in_fmt, pairs in found:
        S = torch.from_numpy(np.stack([np.asarray(openImage(s), dtype=np.float32) for _, s, _ in pairs])).to(dev)
        R = torch.from_numpy(np.stack([np.asarray(openImage(r), dtype=np.float32) for _, _, r in pairs])).to(dev)
        res = retrieve({p: (S[i:i + 1], R[i:i + 1]) for i, (p, _, _) in enumerate(pairs)}, params, **how)[0]
        written += save_retrieval(res, d, exp_id, fmt or in_fmt)
    return written


def retrieve_run_dir(run_dir, params=None, max_shift=None, fmt=None, dark_field=False, method='lcs', window=2, search=3):
    """discover() + lcs (+ integrate when params are given) + save_retrieval for every bin directory; returns the paths.
    dark_field: LCS-DF (4 positions or more), df (+ scattering with params) written too.  method='umpa' (window, search):
    UMPA instead of LCS, 1 position or more, residual written too; method='umpa-df': visibility as well."""
    return _retrieve_found(discover(run_dir, min_positions=_first_floor(method)), params, fmt, max_shift=max_shift,
                           dark_field=dark_field, method=method, window=window, search=search)


def add_retrieval_options(ap):
    """--max-shift, --dark-field, --method, --window, --search on an argparse parser: the retrieval options of this module's
    command line and of main.py's --retrieve."""
    ap.add_argument("--max-shift", type=float, default=None, help="--method lcs: clamp of dx, dy in pixels")
    ap.add_argument("--dark-field", action="store_true",
                    help="--method lcs: LCS-DF (4 positions or more): also df (detector px^2) and, with the physical "
                         "parameters, scattering (rad)")
    ap.add_argument("--method", choices=METHODS, default="lcs",
                    help="lcs (3 positions or more, |D| < 1 px), umpa (1 position or more, |D| up to --search px; also residual) "
                         "or umpa-df (umpa with its dark-field term: also visibility)")
    ap.add_argument("--window", type=int, default=2, help="--method umpa, umpa-df: half-width w of the (2w+1)^2 window, 1..%d"
                    % _lib.PSX_MAX_UMPA_WINDOW)
    ap.add_argument("--search", type=int, default=3, help="--method umpa, umpa-df: largest integer shift searched, 1..%d"
                    % _lib.PSX_MAX_UMPA_SEARCH)


def check_retrieval_options(ap, a, positions=None):
    """The rules of add_retrieval_options' five, as ap.error: which options the method takes, the bounds of --window and --search
    and, where the positions are known (positions: (directory, count) pairs), how many the tracker needs."""
    options = TRACKERS[(a.method, False)].options
    if 'max_shift' not in options and (a.dark_field or a.max_shift is not None):
        ap.error("--dark-field and --max-shift are options of --method lcs")
    wmax, smax = _lib.PSX_MAX_UMPA_WINDOW, _lib.PSX_MAX_UMPA_SEARCH
    if 'window' in options and not (1 <= a.window <= wmax and 1 <= a.search <= smax):
        ap.error("--window and --search must be in 1..%d" % wmax + (" and 1..%d" % smax) * (smax != wmax))
    least = TRACKERS[(a.method, a.dark_field)].min_positions
    for d, n in positions or ():
        if n < least:
            ap.error("--dark-field needs at least %d positions; %s has %d" % (least, d, n))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m paresis_amd.retrieval", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("run_dir")
    ap.add_argument("--energy", type=float, default=None, help="photon energy, keV")
    ap.add_argument("--pixel-um", type=float, default=None, help="detector pixel size, micrometres")
    ap.add_argument("--distance", type=float, default=None, help="object-to-detector distance, metres")
    ap.add_argument("--magnification", type=float, default=None, help="exp_dict['magnification']")
    ap.add_argument("--format", default=None, help="output format (.tif, .edf, .npy); default: the input's")
    ap.add_argument("--propagation", action="store_true",
                    help="Paganin retrieval of each bin's propagation image over its flat field instead of speckle tracking: "
                         "propag/retrieval/{contact,thickness,phi}; needs --delta, --beta and the four physical parameters")
    ap.add_argument("--delta", type=float, default=None, help="--propagation: the sample material's delta at --energy")
    ap.add_argument("--beta", type=float, default=None, help="--propagation: the sample material's beta at --energy")
    add_retrieval_options(ap)
    a = ap.parse_args(argv)
    phys = (a.energy, a.pixel_um, a.distance, a.magnification)
    if a.propagation:
        if any(getattr(a, k) != ap.get_default(k) for k in ("max_shift", "dark_field", "method", "window", "search")):
            ap.error("--propagation takes none of the tracker options (--max-shift, --dark-field, --method, --window, --search)")
        if a.delta is None or a.beta is None or any(v is None for v in phys):
            ap.error("--propagation needs --delta, --beta, --energy, --pixel-um, --distance and --magnification")
        params = {'energy_keV': a.energy, 'pixel_um': a.pixel_um, 'distance_m': a.distance, 'magnification': a.magnification}
        try:
            paganin_alpha(a.delta, a.beta, a.energy, a.pixel_um, a.distance, a.magnification)
        except ValueError as exc:
            ap.error(str(exc))
        for p in retrieve_propagation_run_dir(a.run_dir, params, a.delta, a.beta, fmt=a.format):
            print(p)
        return 0
    if a.delta is not None or a.beta is not None:
        ap.error("--delta and --beta are options of --propagation")
    check_retrieval_options(ap, a)
    if any(v is not None for v in phys) and any(v is None for v in phys):
        ap.error("--energy, --pixel-um, --distance and --magnification go together")
    params = None if phys[0] is None else {'energy_keV': a.energy, 'pixel_um': a.pixel_um, 'distance_m': a.distance,
                                           'magnification': a.magnification}
    found = discover(a.run_dir, min_positions=_first_floor(a.method))
    check_retrieval_options(ap, a, [(d, len(pairs)) for d, _, _, pairs in found])
    for p in _retrieve_found(found, params, a.format, max_shift=a.max_shift, dark_field=a.dark_field, method=a.method,
                             window=a.window, search=a.search):
        print(p)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Spectral material decomposition of energy-binned runs: the inverse of what the source's spectrum and the photon-counting
detector's bins simulate.

A bin of a polychromatic run is beam-hardened: -ln(Propag/White) of it is no line integral of any mu, and treating the bins
as unrelated monochromatic images (retrieval, tomography) ignores what they share.  Projection-domain decomposition takes
the B per-bin log-transmissions of a pixel together and, with the run's own spectrum and the materials' attenuation
coefficients, recovers each material's thickness, beam hardening included:

    L_b = -ln sum_e w_be exp(-sum_m a_m(E_be) t_m)

    model_of(experiment, materials)     the SpectralModel of a run: bins, flat-field weights w, coefficients a (no GPU)
    SpectralModel(names, energies_per_bin, weights, coefficients)     the same, built directly
    transmission(model, thickness)      the forward model, [B, ...] float32 (torch, float64 inside; not a hot path)
    decompose(logT, model, ...)         the per-pixel nonlinear least-squares solve on the GPU (csrc/decompose.hip,
                                        ops.decompose; the contract is in include/paresis_hip.h) -> thickness per material
    monochromatic(thickness, model_or_sample, energy_keV)     the virtual monoenergetic -ln T = sum_m a_m(E) t_m
    scan(experiment, angles_deg, ...)   tomography.scan's per-bin -ln(P/W) sinograms, decomposed into one thickness sinogram
                                        per material
    reconstruct(scanned, ...)           tomography of those: one volume-fraction image per material
    decompose_run(results, model, ...)  main.run's position 0 (Propag and White stacks) decomposed; save_decomposition writes it

    python -m paresis_amd.main --decompose [--decompose-materials A,B] ...

The materials must differ in how their attenuation depends on the energy: the synthetic stand-ins of the shipped
materials (materials.py) all scale as E^-3, so any two of them are proportional and no spectrum can tell them apart.
"""
import os

import numpy as np

from . import _lib

CONDITION_LIMIT = 1e8
ITERATIONS, TOL = 12, 1e-13        # decompose's defaults: the most steps of a pixel, and the change of -ln T it stops at


class SpectralModel:
    """names: the M materials; energies_per_bin: B sequences of energies in keV; weights: B sequences, the flat field's
    per-energy share of each bin (each summing to 1); coefficients: [M][E] linear attenuation coefficients in 1/m over the
    energies of all bins in order, E = the total number of energies.  Host numbers only."""

    def __init__(self, names, energies_per_bin, weights, coefficients):
        self.names = tuple(str(n) for n in names)
        self.energies = [np.asarray(e, dtype=np.float64).ravel() for e in energies_per_bin]
        self.bin_size = [int(e.size) for e in self.energies]
        w = [np.asarray(x, dtype=np.float64).ravel() for x in weights]
        if len(w) != len(self.energies) or any(a.size != b.size for a, b in zip(w, self.energies)):
            raise ValueError("weights must hold one value per energy of every bin")
        if not self.bin_size or min(self.bin_size) < 1:
            raise ValueError("every bin needs one energy at least")
        self.weights = w
        self.w = np.concatenate(w)
        self.a = np.atleast_2d(np.asarray(coefficients, dtype=np.float64))
        E = sum(self.bin_size)
        if self.a.shape != (len(self.names), E):
            raise ValueError("coefficients must be [%d materials][%d energies], got %s" % (len(self.names), E, self.a.shape))
        if not (np.isfinite(self.w).all() and np.isfinite(self.a).all() and (self.w >= 0).all()):
            raise ValueError("weights must be finite and >= 0, coefficients finite")
        for b, x in enumerate(w):
            if abs(x.sum() - 1.0) > 1e-9:
                raise ValueError("the weights of bin %d sum to %r, not 1" % (b, float(x.sum())))
        M, B = len(self.names), len(self.bin_size)
        if not 1 <= M <= _lib.PSX_DECOMP_MAX_MAT:
            raise ValueError("a model takes 1 to %d materials, got %d" % (_lib.PSX_DECOMP_MAX_MAT, M))
        if B > _lib.PSX_DECOMP_MAX_BINS or E > _lib.PSX_DECOMP_MAX_ENERGIES:
            raise ValueError("a model takes %d bins and %d energies at most, got %d and %d"
                             % (_lib.PSX_DECOMP_MAX_BINS, _lib.PSX_DECOMP_MAX_ENERGIES, B, E))
        if B < M:
            raise ValueError("%d materials cannot be told apart from %d energy bins: as many bins as materials are needed, or more"
                             % (M, B))

    @property
    def bins(self):
        return len(self.bin_size)

    def effective(self):
        """Abar [B, M]: the bins' effective coefficients sum_e w_be a_m(E_be), those of an infinitely thin sample."""
        out, e0 = np.zeros((self.bins, len(self.names))), 0
        for b, ne in enumerate(self.bin_size):
            out[b] = self.a[:, e0:e0 + ne] @ self.w[e0:e0 + ne]
            e0 += ne
        return out

    def condition(self):
        """The condition number of Abar with every column scaled to unit length: what decides whether the materials can be
        told apart, whatever their units.  inf for a zero column."""
        A = self.effective()
        norm = np.linalg.norm(A, axis=0)
        if not (norm > 0).all():
            return float("inf")
        return float(np.linalg.cond(A / norm))

    def check_rank(self):
        c = self.condition()
        if not c <= CONDITION_LIMIT:
            raise ValueError("materials %s cannot be told apart in these bins: the column-normalised effective coefficients "
                             "have condition number %.3g > %g.  Materials whose attenuation has the same energy dependence are "
                             "proportional -- the synthetic stand-ins of the shipped materials all scale as E^-3 and are "
                             "rank-deficient by construction" % (", ".join(self.names), c, CONDITION_LIMIT))
        return c

    def linear_start(self, v):
        """G [M, B] = (Abar^T V Abar)^-1 Abar^T V: the least-squares solution of the linearised problem."""
        A, V = self.effective(), np.diag(np.asarray(v, dtype=np.float64))
        return np.linalg.solve(A.T @ V @ A, A.T @ V)

    def coefficients_at(self, energy_keV):
        """a_m at one energy of the model's own (exact match)."""
        E = np.concatenate(self.energies)
        hit = np.nonzero(E == float(energy_keV))[0]
        if hit.size == 0:
            raise ValueError("%r keV is not one of the model's energies" % (energy_keV,))
        return self.a[:, hit[0]]


def _uniform(sample, what):
    """The single value of each map of a uniform thickness stack (air, plate)."""
    g = sample.myGeometry
    g = g.detach().cpu().numpy() if hasattr(g, "detach") else np.asarray(g)
    if g.ndim != 3 or g.shape[0] != len(sample.myMaterials):
        raise ValueError("the %s's geometry must be [material, x, y], got shape %s" % (what, g.shape))
    vals = g.reshape(g.shape[0], -1)
    if not (vals == vals[:, :1]).all():
        raise ValueError("the %s's thickness map is not uniform: the flat field's spectrum would differ from pixel to pixel" % what)
    return vals[:, 0].astype(np.float64)


def model_of(experiment, materials=None):
    """The SpectralModel of an Experiment: its detector bins (Experiment._bins_of_spectrum; energies after the last threshold
    are never detected and are dropped), per bin the flat field's per-energy share -- Experiment._incident times the air's
    and the plate's attenuation at that energy, normalised --, and a_m(E) = -catt of mySampleofInterest.stack_rt(E,
    phase=False), a scattering material's volume fraction included.  materials: the sample's materials to decompose into,
    all by default, 4 at most.  ValueError: an unknown material, a bin no energy closes, an air or plate map that is not
    uniform, fewer bins than materials, materials that cannot be told apart.  Needs no GPU."""
    sample = experiment.mySampleofInterest
    have = list(sample.myMaterials)
    names = have if materials is None else [str(m) for m in materials]
    for nm in names:
        if nm not in have:
            raise ValueError("material %r is not one of the sample of interest's (%s)" % (nm, ", ".join(map(str, have))))
    if len(set(names)) != len(names) or not names:
        raise ValueError("materials must name each material once and one at least, got %r" % (names,))
    if len(names) > _lib.PSX_DECOMP_MAX_MAT:
        raise ValueError("a decomposition takes %d materials at most, got %d: name a subset" % (_lib.PSX_DECOMP_MAX_MAT, len(names)))
    nbins = experiment._close_bins()
    bins, _ = experiment._bins_of_spectrum()
    if len(bins) < nbins:
        raise ValueError("detector bin %d is closed by no energy of the spectrum (thresholds denser than the sampling)" % len(bins))
    if len(bins) < len(names):
        raise ValueError("%d materials cannot be told apart from %d energy bins: as many bins as materials are needed, or more"
                         % (len(names), len(bins)))
    air = None if experiment.exp_dict['inVacuum'] else experiment.myAirVolume
    plate = experiment.myPlate
    flat = [(o, _uniform(o, nm)) for o, nm in ((air, "air volume"), (plate, "plate")) if o is not None]
    rows = [have.index(nm) for nm in names]
    energies, weights, coeffs = [], [], []
    for energies_of_bin in bins:
        w = []
        for ie, E, flux in energies_of_bin:
            I = experiment._incident(flux, E, ie)
            for o, t in flat:
                I *= float(np.exp(np.dot(o.coeffs_rt(E, phase=False)[1], t)))
            w.append(I)
            coeffs.append(-np.asarray(sample.coeffs_rt(E, phase=False)[1])[rows])
        w = np.asarray(w, dtype=np.float64)
        if not w.sum() > 0:
            raise ValueError("the flat field of the bin ending at %r keV is empty" % (energies_of_bin[-1][1],))
        energies.append([E for _, E, _ in energies_of_bin])
        weights.append(w / w.sum())
    model = SpectralModel(names, energies, weights, np.stack(coeffs, axis=1))
    model.check_rank()
    return model


def transmission(model, thickness):
    """The forward model: thickness [M, ...] (metres; a tensor on any device, or an array) -> T [B, ...] float32 on the same
    device, T_b = sum_e w_be exp(-sum_m a_m(E_be) t_m), in float64 inside."""
    import torch
    t = torch.as_tensor(thickness)
    if t.shape[0] != len(model.names):
        raise ValueError("thickness must be [%d, ...], got shape %s" % (len(model.names), tuple(t.shape)))
    t = t.to(torch.float64)
    a = torch.as_tensor(model.a, device=t.device)
    w = torch.as_tensor(model.w, device=t.device)
    out, e0 = [], 0
    for ne in model.bin_size:
        ex = torch.exp(-torch.tensordot(a[:, e0:e0 + ne].T.contiguous(), t, dims=1))      # [ne, ...]
        out.append(torch.tensordot(w[e0:e0 + ne], ex, dims=1))
        e0 += ne
    return torch.stack(out).to(torch.float32)


def _bin_weights(model, weights):
    v = np.ones(model.bins) if weights is None else np.asarray(weights, dtype=np.float64).ravel()
    if v.size != model.bins or not (np.isfinite(v).all() and (v > 0).all()):
        raise ValueError("weights must hold one finite value > 0 per bin (%d), got %r" % (model.bins, weights))
    return v


def decompose(logT, model, iterations=ITERATIONS, tol=TOL, weights=None):
    """logT: [B, ...] float32 CUDA tensor (or a sequence of B equal-shaped ones), L_b = -ln of bin b's transmission, of any
    trailing shape -- a whole sinogram stack goes through in one launch -> {'thickness': [M, ...] metres, 'residual':
    [...] sqrt(sum_b v_b r_b^2) at the solution, 'steps': [...] Gauss-Newton steps taken (-1: a value that is not finite,
    thickness 0 and residual inf; -2: the normal matrix was not positive definite, the last x is kept)}, float32.
    iterations: the most steps a pixel takes; tol: it stops when the step's largest change of -ln T falls to tol;
    weights: one per bin (v_b > 0; ones by default; 1/variance of L_b is the statistical choice).  The thickness is not
    clamped: noise gives negative values, and clamping would bias their mean."""
    from . import ops
    model.check_rank()
    v = _bin_weights(model, weights)
    t, r, s = ops.decompose(logT, model.bin_size, model.w, model.a, v, model.linear_start(v), iterations=iterations, tol=tol)
    return {'thickness': t, 'residual': r, 'steps': s}


def monochromatic(thickness, model_or_sample, energy_keV):
    """The virtual monoenergetic image of decomposed thicknesses [M, ...]: -ln T = sum_m a_m(E) t_m.  model_or_sample: a
    SpectralModel (E must be one of its energies) or the sample of interest, whose materials are then the thicknesses' in
    order and whose coefficient table holds E."""
    if isinstance(model_or_sample, SpectralModel):
        a = model_or_sample.coefficients_at(energy_keV)
    else:
        a = -np.asarray(model_or_sample.coeffs_rt(float(energy_keV), phase=False)[1], dtype=np.float64)
    if thickness.shape[0] != len(a):
        raise ValueError("thickness must be [%d, ...], got shape %s" % (len(a), tuple(thickness.shape)))
    out = thickness[0] * float(a[0])
    for m in range(1, len(a)):
        out = out + thickness[m] * float(a[m])
    return out


def scan(experiment, angles_deg, materials=None, **decompose_options):
    """tomography.scan(experiment, angles_deg) -- the chain once per angle, -ln(Propag/White) per bin, which is exactly L_b
    -- decomposed, each whole [B, A, n, m] stack in one launch -> {'sinograms': {material name: [A, n, m] thickness in
    metres}, 'residual': [A, n, m], 'angles', 'center', 'voxel_m', 'modality': 'materials'}.  materials: model_of's;
    decompose_options: decompose's iterations, tol, weights.  The model's errors are raised before the chain runs."""
    import torch
    from . import tomography as tomo
    if isinstance(experiment, dict):
        from .Experiment import Experiment
        experiment = Experiment(experiment)
    model = model_of(experiment, materials)
    scanned = tomo.scan(experiment, angles_deg)
    L = torch.stack([scanned['sinograms'][b] for b in range(model.bins)])
    r = decompose(L, model, **decompose_options)
    return {'sinograms': {nm: r['thickness'][m] for m, nm in enumerate(model.names)}, 'residual': r['residual'],
            'angles': scanned['angles'], 'center': scanned['center'], 'voxel_m': scanned['voxel_m'], 'modality': 'materials'}


def reconstruct(scanned, filter='ramp', circle=True, method='fbp', iterations=None, nonneg=False, weight=None):
    """A material scan's volumes -> {material name: [n, m, m] float32 volume fraction} (1 where the voxel is all that
    material): the thickness sinogram is a line integral of the fraction in metres, which tomography.mu_volume's division
    by the voxel turns into the fraction.  method, iterations, nonneg, weight: the rows and rules of
    tomography.RECONSTRUCTIONS (tomography.reconstruct's; weight relative to the sinogram's largest value)."""
    from . import tomography as tomo
    tomo.check_reconstruction(method, iterations, nonneg, weight)
    if scanned.get('modality') != 'materials':
        raise ValueError("spectral.reconstruct takes spectral.scan's result, got modality %r" % (scanned.get('modality'),))
    row = tomo.RECONSTRUCTIONS[method]
    options = {'iterations': iterations} if row.iterations else {'filter': filter}
    if row.nonneg:
        options['nonneg'] = nonneg
    out = {}
    for name, s in scanned['sinograms'].items():
        if row.weight:
            options['weight'] = float(weight) * float(s.abs().max())
        vol = row.solver(s.contiguous(), scanned['angles'], center=scanned['center'], circle=circle, **options)
        out[name] = tomo.mu_volume(vol, scanned['voxel_m'])
    return out


def decompose_run(results, model, device=None, **decompose_options):
    """main.run's {position: (Sample, Reference, Propag, White, ...)}: position 0's [nbins, n, m] Propag and White stacks (host
    or device) -> decompose's dict for L_b = -ln(Propag_b/White_b)."""
    import torch
    from .retrieval import _stack
    if 0 not in results or len(results[0]) < 4:
        raise ValueError("results hold no propagation image: position 0's (Sample, Reference, Propag, White) is needed")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    P, W = _stack(results, [0], 2, dev)[0], _stack(results, [0], 3, dev)[0]
    if P.shape[0] != model.bins:
        raise ValueError("the run has %d bins, the model %d" % (P.shape[0], model.bins))
    return decompose(-torch.log(P / W), model, **decompose_options)


def save_decomposition(r, names, directory, exp_id, fmt):
    """Write directory/propag/materials/thickness_<material>_<exp_id><fmt> per material and residual_<exp_id><fmt>."""
    from .InputOutput.pagailleIO import save_image
    d = os.path.join(directory, "propag", "materials")
    os.makedirs(d, exist_ok=True)
    paths = []
    for m, nm in enumerate(names):
        paths.append(os.path.join(d, "thickness_%s_%s%s" % (nm, exp_id, fmt)))
        save_image(r['thickness'][m].detach().cpu().numpy(), paths[-1])
    paths.append(os.path.join(d, "residual_%s%s" % (exp_id, fmt)))
    save_image(r['residual'].detach().cpu().numpy(), paths[-1])
    return paths

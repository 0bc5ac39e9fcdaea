#!/usr/bin/env python3
"""XML-driven entry point (mirror of CodePython/main.py:20-115).

    python -m paresis_amd.main [--experiment NAME] [--type RayT|Fresnel] [--oversampling N] [--points N]
                               [--out DIR] [--format .tif|.edf|.npy] [--xml DIR] [--no-noise] [--seed S] [--backend nccl|gloo]
                               [--retrieve [--max-shift S] [--dark-field] [--method lcs|umpa|umpa-df --window W --search M]]
                               [--retrieve-propagation [--material NAME]]
                               [--decompose [--decompose-materials A,B]]
                               [--tomography A [--tomography-modality attenuation|phase [--tomography-differential]]
                                [--tomography-method fbp|sirt|cgls|tv --tomography-iterations K [--tomography-weight W]]
                                [--tomography-beam parallel|cone]]

With torchrun (one process per GPU) the membrane positions are strided over the ranks and the detector images are
gathered on rank 0 over RCCL (paresis_amd/dist.py); results do not depend on the number of GPUs because every position
has its own seed.  --retrieve (needs 3 positions or more) runs the speckle-tracking phase retrieval of each bin on rank 0
after the gather (paresis_amd/retrieval.py) and writes retrieval/{transmission,dx,dy,phi}_<expID><fmt> under the bin's
directory.  --dark-field (needs 4 positions or more) retrieves with LCS-DF and adds df_ and scattering_<expID><fmt>.
--method umpa (1 position or more) retrieves with UMPA, for displacements of up to --search pixels, and adds
residual_<expID><fmt>; it takes neither --dark-field nor --max-shift.  --method umpa-df (the same rules) also fits UMPA's
dark-field term and adds visibility_<expID><fmt>.  --retrieve-propagation (independent of --retrieve; any number of
positions) runs Paganin's single-material retrieval of each bin's propagation image over its flat field on rank 0 and writes
propag/retrieval/{contact,thickness,phi}_<expID><fmt> under the bin's directory; --material names the sample material whose
delta and beta the filter takes (default: the sample of interest's first).  --decompose (independent of --retrieve; any number
of positions; a run of several energy bins) decomposes the bins' propagation images over their flat fields into one thickness
map per sample material on rank 0 (paresis_amd/spectral.py: the run's own spectrum and the materials' attenuation, beam
hardening included) and writes propag/materials/thickness_<material>_<expID><fmt> and residual_<expID><fmt> under the first
bin's directory; --decompose-materials names the materials to decompose into (default: all of the sample's).  --tomography A (samples that are the contrast
phantom or a getVolumeFromFile label volume) then turns the sample through A angles on [0, 180) degrees, runs the chain at
each (paresis_amd/tomography.py scan),
reconstructs by filtered back-projection on rank 0 and writes tomography/mu_<expID> (--tomography-modality attenuation,
the default: 1/m, from -ln(Propag/White), any --points) or tomography/delta_<expID> (phase: from the retrieved phi, the
rules and options of --retrieve) under each bin's directory: one [n, m, m] file for --format .npy, else a directory of
slices.  --tomography-method sirt|cgls reconstructs with --tomography-iterations K >= 1 steps of SIRT or CGLS on the matched
projector pair instead (tomography.sirt / cgls): the methods for few angles.  --tomography-method tv takes K steps of
total-variation reconstruction (tomography.tv) with --tomography-weight W >= 0, relative to the sinogram's largest value: the
model of the phantom's piecewise constant slices, for fewer angles still.  --tomography-differential (with
--tomography-modality phase and --tomography-method fbp only) skips the phase integration: the tracked gradient across the
rotation axis is back-projected through a Hilbert filter, and tomography/delta_<expID> is written as before.
--tomography-beam cone (a getVolumeFromFile sample, --tomography-method fbp, no --tomography-differential) projects the volume
from the experiment's point source instead -- distSourceToMembrane + distMembraneToObject from the rotation axis --, takes
the A angles on [0, 360) and reconstructs by FDK.
"""
import argparse
import datetime
import os
import time

import numpy as np


def run(exp_dict, save=True, saving_format=".tif", backend=None, retrieve=False, max_shift=None, dark_field=False,
        method='lcs', window=2, search=3, propagation=False, material=None, tomography=0, tomography_modality='attenuation',
        tomography_method='fbp', tomography_iterations=0, tomography_weight=None, tomography_differential=False,
        decompose=False, decompose_materials=None, tomography_beam='parallel'):
    """main.py:58-115.  Returns on rank 0 {position: (Sample, Reference[, Propag, White, ...])} with host tensors.

    retrieve (extension): rank 0 retrieves every bin from the run's own positions after the gather
    (retrieval.retrieve with the experiment's parameters, max_shift its clamp); with save, the maps go to
    <bin dir>/retrieval/.  exp_dict['retrievalParams'] then holds the parameters it used.  dark_field (with retrieve, 4
    positions or more): LCS-DF, the maps gain df and scattering (retrieval.retrieve(..., dark_field=True)).  method='umpa'
    (with retrieve, 1 position or more; window, search as retrieval.umpa): UMPA instead of LCS, the maps gain residual;
    method='umpa-df' (the same rules): UMPA with its dark-field term, the maps gain visibility and residual.

    propagation (extension, independent of retrieve, any number of positions): rank 0 also retrieves every bin's
    propagation image over its flat field with Paganin's filter (retrieval.retrieve_propagation with the experiment's
    parameters and the delta, beta of `material` -- retrieval.propagation_material: by default the sample of interest's
    first); with save, contact, thickness and phi go to <bin dir>/propag/retrieval/.  exp_dict['propagationParams'] then
    holds the parameters, the material and the delta, beta, alpha and mu it used.

    decompose (extension, independent of retrieve, any number of positions): rank 0 also decomposes the bins of position
    0's propagation image over its flat field into the thicknesses of decompose_materials (the sample of interest's
    materials, all by default; spectral.model_of and spectral.decompose_run); a model that cannot be decomposed -- fewer
    bins than materials, materials of one energy dependence -- is a ValueError before the images are computed.  With save,
    <first bin dir>/propag/materials/ gets thickness_<material>_ and residual_<expID><fmt>.  exp_dict['decomposeParams']
    then holds the materials, the bins' energies and weights and the model's condition number, and
    exp_dict['decomposition'] the {'thickness', 'residual', 'steps'} device tensors.

    tomography = A > 0 (extension; the sample of interest must be the contrast phantom or a getVolumeFromFile label
    volume): after the run, rank 0 turns it through A angles on [0, 180), runs the chain at each (tomography.scan with
    tomography_modality; 'phase'
    retrieves with method, max_shift, dark_field, window, search and needs their positions), reconstructs every bin
    (tomography.reconstruct) and, with save, writes <bin dir>/tomography/{mu|delta}_<expID> (tomography.save_volume).
    tomography_method 'sirt' or 'cgls' with tomography_iterations >= 1 reconstructs iteratively instead of by filtered
    back-projection ('fbp', which takes no iterations); 'tv' with tomography_iterations >= 1 and tomography_weight >= 0
    (relative to the sinogram's largest value, as tomography.reconstruct takes it; refused for the other methods)
    reconstructs with total variation.  tomography_differential (modality 'phase' and method 'fbp' only): the scan keeps
    the tracked gradient across the rotation axis instead of the integrated phase (tomography.scan(..., differential=True))
    and the reconstruction goes through the Hilbert filter.  tomography_beam 'cone' (a label volume, method 'fbp', not
    differential): the volume is projected from the experiment's point source (tomography.scan(..., beam='cone')), the A
    angles lie on [0, 360) and the reconstruction is FDK; tomographyParams then also holds 'beam', 'source_px' and
    'row_center'.  exp_dict['tomographyParams'] then holds the angles, the centre,
    the voxel size, the modality, whether the scan was differential, the method, its iterations and its weight (None but for
    'tv'), and exp_dict['tomographyVolumes'] the {bin: [n, m, m] device tensor} volumes."""
    from . import tomography as tomo
    tomo.check_run_options(tomography, tomography_modality, tomography_method, tomography_iterations, tomography_weight,
                           differential=tomography_differential, beam=tomography_beam)
    if tomography and tomography_modality == 'phase':
        from .retrieval import check_method
        check_method(method, int(exp_dict['nbExpPoints']), max_shift, dark_field)
    if material is not None and not propagation:
        raise ValueError("material is an option of propagation")
    if decompose_materials is not None and not decompose:
        raise ValueError("decompose_materials is an option of decompose")
    if retrieve and method != "lcs":
        from .retrieval import check_method
        check_method(method, int(exp_dict['nbExpPoints']), max_shift, dark_field)
    elif retrieve and int(exp_dict['nbExpPoints']) < 3:
        raise ValueError("--retrieve needs at least 3 membrane positions, got %d" % int(exp_dict['nbExpPoints']))
    if dark_field and not retrieve:
        raise ValueError("dark_field is an option of retrieve")
    if dark_field and int(exp_dict['nbExpPoints']) < 4:
        raise ValueError("dark-field retrieval needs at least 4 membrane positions, got %d" % int(exp_dict['nbExpPoints']))
    from . import dist
    from .Experiment import Experiment
    from .InputOutput.pagailleIO import save_image

    time0 = time.time()
    rank, world = dist.init(backend)
    # one experiment ID for all ranks (the reference takes the wall clock, main.py:30; ranks would disagree by a second)
    exp_dict['expID'] = dist.broadcast_object(datetime.datetime.now().strftime("%Y%m%d-%H%M%S"), rank, world)
    exp_dict.setdefault('deferMeanEnergy', True)       # no host synchronisation per position (resolved before the dump)
    # this loop only reads the stacks a position returns (packs, copies to the host, saves): the all-zero Propag / White of the
    # positions after the first may be ONE stack of the experiment (Experiment._begin)
    exp_dict.setdefault('sharedZeroStacks', True)
    # exp_dict['reproducible'] (default True; --float-atomics turns it off): the ray-tracing chain's far rays go through the
    # order-independent replay (the Experiment class sets psx_set_deterministic around its chain and restores the caller's
    # mode): every image is then the same bits on 1 GPU and on 8; the Fresnel chain has no float atomics and is reproducible
    # as it is
    print("\n\nINITIALIZING EXPERIMENT PARAMETERS AND GEOMETRIES")
    experiment = Experiment(exp_dict)
    if propagation:
        from .retrieval import propagation_material
        material = propagation_material(experiment, material)       # a wrong name fails before the images are computed
    if decompose:
        from . import spectral
        spectral_model = spectral.model_of(experiment, decompose_materials)   # a model error fails before the images are computed
    if tomography:
        tomo._phantom(experiment.mySampleofInterest)                # another sample fails before the images are computed
        if tomography_beam == 'cone':
            tomo.check_diverging(experiment.mySampleofInterest)     # and so does a sample that cannot diverge
    sim = exp_dict['simulation_type']
    root = exp_dict['filepath'] + ('Fresnel_' if sim == "Fresnel" else 'RayTracing_') + str(exp_dict['expID']) + '/'
    if save:
        if rank == 0:
            os.makedirs(root + 'membraneThickness/', exist_ok=True)                       # main.py:84-85
        dist.barrier()
    # everything allocated so far lives as long as the run: keep it out of the cyclic garbage collector's generations, or a
    # full collection (tens of ms with the GPU idle) lands in one of the first positions
    import gc
    gc.collect()
    gc.freeze()
    print("\nImages calculation")
    # the detector stacks go to rank 0 round by round while the next positions are computed (dist.PositionGatherer); the
    # Fresnel plan then hands out its line groups through a queue, so that the transfer's copy kernels cost it a few per cent
    dims = experiment.myDetector.det_param["myDimensions"]
    # Without shot noise the images are not photon counts: the packed 16-bit rounds would all be flagged and the gather
    # repeated in float32 at the end -- one float32 gather at the end from the start, then.  The overlapped form also needs
    # its buffers on every rank: rank 0 alone holds the receive buckets, so whether they could be allocated is decided
    # TOGETHER (a rank that fell back on its own would issue different collectives from the others and hang them).
    overlapped = world > 1 and bool(exp_dict.get('noise', True))
    gatherer = None
    if overlapped:
        gatherer = dist.PositionGatherer(exp_dict['nbExpPoints'], rank, world, to_host=True,
                                         shape=(experiment._close_bins(), int(dims[0]), int(dims[1])))
        if not dist.agree_on_overlap(gatherer):
            overlapped, gatherer = False, None
    if overlapped and sim == "Fresnel":
        experiment._plan().work_queue(True)
    experiment.reserve_outputs(len(dist.my_positions(exp_dict['nbExpPoints'], rank, world)) + 1)   # no hipMalloc inside the loop
    results = {}
    # the loop and the final gather share ONE failure path: PositionGatherer.add() issues collectives too, and a DistError
    # raised there must not unwind through the process group's teardown (its contract: leave with os._exit)
    try:
        for pointNum in dist.my_positions(exp_dict['nbExpPoints'], rank, world):
            experiment.myMembrane.myGeometry = []
            experiment.myMembrane.getMyGeometry(experiment.exp_dict['studyDimensions'], experiment.myMembrane.membranePixelSize,
                                                experiment.exp_dict['overSampling'], pointNum, exp_dict['nbExpPoints'])   # main.py:64-65
            print("\nCalculations point", pointNum)
            out = experiment.computeSampleAndReferenceImages(pointNum)
            if gatherer is not None:
                gatherer.add(pointNum, out)
            else:
                results[pointNum] = out
            if save and exp_dict.get('saveMembrane', True):
                # main.py:98: every rank writes the membrane maps of its own positions (one node, one file system: no gather)
                save_image(experiment.myMembrane.myGeometry[0], root + 'membraneThickness/' + exp_dict['experimentName'] +
                           '_sampling' + str(exp_dict['overSampling']) + '_' + str(pointNum) + saving_format)
        if gatherer is not None:
            gathered = gatherer.finish()
        else:
            gathered = dist.gather_positions(results, exp_dict['nbExpPoints'], rank, world, to_host=True,
                                             pack=bool(exp_dict.get('noise', True)))
    except dist.DistError as exc:             # the ranks are out of step: no further collective can be trusted
        import sys
        import traceback
        traceback.print_exc()
        sys.stderr.write("paresis_amd.main: %s -- leaving\n" % exc)
        sys.stderr.flush()
        os._exit(6)
    finally:
        gc.unfreeze()                         # run() is also an API: leave the collector as it was found
    experiment.resolve_mean_energy()
    if rank == 0 and save:
        os.makedirs(root, exist_ok=True)
        thresholds = [experiment.mySource.mySpectrum[0][0]] + list(experiment.myDetector.det_param['myBinsThersholds'])
        nbin = gathered[0][0].shape[0]
        paths = []
        for ibin in range(nbin):                                         # main.py:84-96
            p = root if nbin == 1 else f'{root}{"%2.2d" % thresholds[ibin]}_{"%2.2d" % thresholds[ibin + 1]}kev/'
            for sub in ("ref/", "sample/", "propag/"):
                os.makedirs(p + sub, exist_ok=True)
            paths.append(p)
        if sim == "RayT":
            # main.py:100-101 writes Df after every position to the SAME file: what stays is the last position's, which is
            # all zeros unless that position is 0 (darkFieldPropag only builds up there, EXP:491)
            N = tuple(int(v) for v in experiment.exp_dict['studyDimensions'])
            last = exp_dict['nbExpPoints'] - 1
            df = gathered[0][6] if last == 0 and len(gathered[0]) > 6 else np.zeros(N, dtype=np.float32)
            save_image(df, root + "DF" + saving_format)
        for pointNum in sorted(gathered):
            S, R = gathered[pointNum][0], gathered[pointNum][1]
            txt = '%2.2d' % pointNum
            for ibin in range(nbin):
                save_image(S[ibin], paths[ibin] + 'sample/sampleImage_' + str(exp_dict['expID']) + '_' + txt + saving_format)
                save_image(R[ibin], paths[ibin] + 'ref/ReferenceImage_' + str(exp_dict['expID']) + '_' + txt + saving_format)
                if pointNum == 0 and len(gathered[0]) > 3:
                    save_image(gathered[0][2][ibin], paths[ibin] + 'propag/PropagImage_' + str(exp_dict['expID']) + '_' + saving_format)
                    save_image(gathered[0][3][ibin], paths[ibin] + 'White_' + str(exp_dict['expID']) + '_' + saving_format)
        experiment.saveAllParameters(time0, exp_dict)
    if rank == 0 and retrieve:
        from . import retrieval
        params = retrieval.params_from_experiment(experiment)
        retrieved = retrieval.retrieve(gathered, params, max_shift=max_shift, dark_field=dark_field, method=method,
                                       window=window, search=search)
        exp_dict['retrievalParams'] = params
        if save:
            for ibin in sorted(retrieved):
                retrieval.save_retrieval(retrieved[ibin], paths[ibin], exp_dict['expID'], saving_format)
    if rank == 0 and propagation:
        from . import materials, retrieval
        params = retrieval.params_from_experiment(experiment)
        delta, beta = materials.delta_beta(material, params['energy_keV'])      # every bin at the run's mean energy, as retrieve
        alpha, mu = retrieval.paganin_alpha(delta, beta, **params)
        propagated = retrieval.retrieve_propagation(gathered, params, (delta, beta))
        exp_dict['propagationParams'] = dict(params, material=material, delta=delta, beta=beta, alpha=alpha, mu=mu)
        if save:
            for ibin in sorted(propagated):
                retrieval.save_propagation(propagated[ibin], paths[ibin], exp_dict['expID'], saving_format)
    if rank == 0 and decompose:
        decomposed = spectral.decompose_run(gathered, spectral_model)
        exp_dict['decomposeParams'] = {'materials': list(spectral_model.names), 'energies_keV': [e.tolist() for e in spectral_model.energies],
                                       'weights': [w.tolist() for w in spectral_model.weights], 'condition': spectral_model.condition(),
                                       'iterations': spectral.ITERATIONS, 'tol': spectral.TOL}
        exp_dict['decomposition'] = decomposed
        if save:
            spectral.save_decomposition(decomposed, spectral_model.names, paths[0], exp_dict['expID'], saving_format)
    if rank == 0 and tomography:
        turn = 360.0 if tomography_beam == 'cone' else 180.0
        angles = [turn * a / int(tomography) for a in range(int(tomography))]
        options = {}
        if tomography_modality == 'phase':
            from .retrieval import TRACKERS
            options = {'method': method, 'max_shift': max_shift, 'dark_field': dark_field, 'window': window, 'search': search}
            keep = TRACKERS[(method, bool(dark_field))].options + ('method', 'dark_field')
            options = {k: v for k, v in options.items() if k in keep}
            if tomography_differential:
                options['differential'] = True
        if tomography_beam != 'parallel':
            options['beam'] = tomography_beam
        scanned = tomo.scan(experiment, angles, modality=tomography_modality, **options)
        volumes = tomo.reconstruct(scanned, method=tomography_method, iterations=tomography_iterations or None,
                                   weight=tomography_weight)
        exp_dict['tomographyParams'] = {k: scanned[k] for k in ('angles', 'center', 'voxel_m', 'modality', 'differential', 'energy_keV',
                                                                 'beam', 'source_px', 'row_center') if k in scanned}
        exp_dict['tomographyParams'].update(method=tomography_method, iterations=int(tomography_iterations),
                                             weight=None if tomography_weight is None else float(tomography_weight))
        if save:
            nbin = len(volumes)
            thresholds = [experiment.mySource.mySpectrum[0][0]] + list(experiment.myDetector.det_param['myBinsThersholds'])
            for ibin in sorted(volumes):
                p = root if nbin == 1 else f'{root}{"%2.2d" % thresholds[ibin]}_{"%2.2d" % thresholds[ibin + 1]}kev/'
                tomo.save_volume(volumes[ibin], p + 'tomography/' + tomo.volume_name(tomography_modality) + '_' +
                                 str(exp_dict['expID']), saving_format)
        exp_dict['tomographyVolumes'] = volumes
    dist.finish()
    print("\nfini")
    return gathered


def main(argv=None):
    from . import retrieval, tomography as tomo
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--experiment", default="Fil_Nylon_ID17")
    ap.add_argument("--type", default="RayT", choices=["RayT", "Fresnel"])
    ap.add_argument("--oversampling", type=int, default=2)
    ap.add_argument("--points", type=int, default=1)
    ap.add_argument("--out", default="Results/")
    ap.add_argument("--format", default=".tif")
    ap.add_argument("--xml", default=None)
    ap.add_argument("--no-noise", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reproducible", action="store_true", help="accepted and ignored: the default since round 5")
    ap.add_argument("--float-atomics", action="store_true",
                    help="ray tracing: far rays summed with float atomics in arrival order (a few per cent faster; the last bit of "
                         "an image, and with it a Poisson draw, may differ between runs and GPU counts)")
    ap.add_argument("--backend", default=None, choices=[None, "nccl", "gloo"],
                    help="torch.distributed backend under torchrun (default: nccl = RCCL on a GPU node; gloo rehearses several "
                         "ranks on one GPU)")
    ap.add_argument("--retrieve", action="store_true",
                    help="speckle-tracking phase retrieval of every bin after the run (3 positions or more): "
                         "retrieval/{transmission,dx,dy,phi}_<expID><fmt> under each bin's directory")
    retrieval.add_retrieval_options(ap)          # --max-shift, --dark-field, --method, --window, --search: options of --retrieve
    ap.add_argument("--retrieve-propagation", action="store_true",
                    help="Paganin retrieval of every bin's propagation image after the run (any --points): "
                         "propag/retrieval/{contact,thickness,phi}_<expID><fmt> under each bin's directory")
    ap.add_argument("--material", default=None,
                    help="--retrieve-propagation: the sample material the filter assumes (default: the sample's first)")
    ap.add_argument("--decompose", action="store_true",
                    help="material decomposition of the energy bins' propagation images after the run (any --points): "
                         "propag/materials/thickness_<material>_<expID><fmt> and residual_<expID><fmt> under the first bin's directory")
    ap.add_argument("--decompose-materials", default=None, metavar="A,B",
                    help="--decompose: the sample materials to decompose into, comma-separated (default: all of the sample's)")
    tomo.add_tomography_options(ap)              # --tomography and its --tomography-modality, -differential, -method, ...
    a = ap.parse_args(argv)
    exp_dict = {'experimentName': a.experiment, 'filepath': a.out if a.out.endswith('/') else a.out + '/',
                'overSampling': a.oversampling, 'nbExpPoints': a.points, 'simulation_type': a.type,
                'noise': not a.no_noise, 'seed': a.seed, 'reproducible': not a.float_atomics}
    if a.xml:
        exp_dict['xmlDir'] = a.xml
    os.makedirs(exp_dict['filepath'], exist_ok=True)
    if a.method != "lcs" and not a.retrieve and a.tomography_modality != "phase":
        ap.error("--method is an option of --retrieve and of --tomography-modality phase")
    retrieval.check_retrieval_options(ap, a)
    floor = {df: t.min_positions for (m, df), t in retrieval.TRACKERS.items() if m == a.method}
    if a.retrieve and a.points < floor[False]:
        ap.error("--retrieve needs --points %d or more" % floor[False])
    if a.dark_field and not a.retrieve:
        ap.error("--dark-field is an option of --retrieve")
    if a.dark_field and a.points < floor[True]:
        ap.error("--dark-field needs --points %d or more" % floor[True])
    if a.material is not None and not a.retrieve_propagation:
        ap.error("--material is an option of --retrieve-propagation")
    if a.decompose_materials is not None and not a.decompose:
        ap.error("--decompose-materials is an option of --decompose")
    tomo.check_tomography_options(ap, a)
    run(exp_dict, save=True, saving_format=a.format, backend=a.backend, retrieve=a.retrieve, max_shift=a.max_shift,
        dark_field=a.dark_field, method=a.method, window=a.window, search=a.search, propagation=a.retrieve_propagation,
        material=a.material, tomography=a.tomography, tomography_modality=a.tomography_modality,
        tomography_method=a.tomography_method, tomography_iterations=a.tomography_iterations,
        tomography_weight=a.tomography_weight, tomography_differential=a.tomography_differential,
        tomography_beam=a.tomography_beam, decompose=a.decompose,
        decompose_materials=None if a.decompose_materials is None else [m.strip() for m in a.decompose_materials.split(",")])


if __name__ == "__main__":
    main()

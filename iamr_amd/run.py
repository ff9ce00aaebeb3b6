"""`python -m iamr_amd.run <inputs file> [key=value ...]` -- IAMR's main loop (Source/main.cpp:60-145: ParmParse, Amr::init,
`while (step < max_step && time < stop_time) coarseTimeStep`) driving libiamrx.so from an unmodified IAMR inputs file (SURVEY row
f4): one level, or a hierarchy of fixed refined grids (amr.max_level > 0 with amr.regrid_file, subcycled, inviscid).  Both go through
ONE start-up sequence and loop (drive) and one plotfile writer (write_plot): a level offers the members of a hierarchy of one
(ns.NavierStokes), and what the two do differently are the four small functions in front of drive.  Under
torch.distributed.run the boxes of every level are spread over the ranks (one process per GPU); plotfiles and checkpoints are written
by all ranks together (every rank the fabs it owns, rank 0 the headers) and amr.restart reads a checkpoint on any number of ranks.
IAMRX_RUN_TRANSPORT=gloo: the ranks talk through torch.distributed's gloo on host buffers and all use device 0 (several ranks on the one
GPU of a test machine); unset: nccl + RCCL, one GPU per rank."""
import os
import sys
import time

from .lib import local_indices          # (which of a layout's boxes this rank owns: callers of level_arrays and write_plot ask here)


def init_level(ns, lay, lib, N, pr, n):
    """initial data of one level (prob_initData role, Source/prob/prob_init.cpp), n = the level's cell counts"""
    pb = pr["prob"]
    if pb["probtype"] == 1:
        ns.init_rest(pb["rho0"])
    elif pb["probtype"] in (2, 4, 5, 6, 7, 100):
        from .probinit import set_initial_state
        ns.init_rest(pb["density_ic"])
        set_initial_state(ns, lay, lib, N, pb, n, pr["prob_lo"], pr["prob_hi"])
    elif pb["probtype"] == 101:
        from .probinit import set_synthetic_state
        ns.init_rest(pb["density_ic"])
        set_synthetic_state(ns, lay, lib, N, pb, n)
    elif pb["probtype"] == 10:
        ns.init_rayleightaylor(pb["rho_1"], pb["rho_2"], pb["tra_1"], pb["tra_2"], pb["pertamp"], pb["interface_width"])
    else:
        ns.init_taylorgreen(pb["vfac"], pb["a"], pb["b"], pb["c"], pb["rho0"])


def solver_opts(pr, lib, **mg_kw):
    """the run's multigrid options.  2-D run on its slab: the multigrid keeps the slab two cells thick (mlmg.hip mg_slab_level) -- a
    property of THIS problem's solvers, handed over in their options (not process-wide tuning: ADVICE round 5)"""
    return lib.mg_opts(slab=1 if pr.get("slab") else 0, **mg_kw)


def level0_geom(pr, lib):
    return lib.Geom.make(pr["n"], prob_lo=pr["prob_lo"], prob_hi=pr["prob_hi"], periodic=pr["periodic"])


def build_amr(pr, lib, N, world=1, **mg_kw):
    """hierarchy of fixed grids: level 0 chopped by amr.max_grid_size, the refined levels as the grid file gives them"""
    from .amr import Amr
    g0 = level0_geom(pr, lib)
    lays = [lib.Layout.decompose(tuple(pr["n"]), pr["max_grid_size"], world)] + [lib.Layout(b, [q % world for q in range(len(b))]) for b in pr["fine_boxes"]]
    amr = Amr(g0, lays, N.ns_params(**pr["params"]), solver_opts(pr, lib, **mg_kw))
    for l, lev in enumerate(amr.levels):
        init_level(lev, lays[l], lib, N, pr, [v * 2 ** l for v in pr["n"]])
    if pr.get("regrid"):
        # Amr::bldFineLevels: the initial hierarchy from the tags of the initial data, one level at a time; the new level's data are
        # the problem's initial data (initData), not the interpolant
        amr.set_regrid(**pr["regrid"])
        # amr.initial_grid_file: the initial hierarchy is the file's, the tags only drive the regrids during the run
        for _ in range(0 if pr["fine_boxes"] else pr["regrid"]["max_level"]):
            nl = amr.nlev
            if not amr.regrid():
                break
            for l in range(1, amr.nlev):
                init_level(amr.levels[l], amr.layouts[l], lib, N, pr, [v * 2 ** l for v in pr["n"]])
            if amr.nlev == nl and amr.nlev > pr["regrid"]["max_level"]:
                break
    return amr, amr.layouts, g0


def build(inp, lib, N, nranks=1, pr=None):
    """one level: the domain chopped by amr.max_grid_size"""
    pr = pr if pr is not None else inp.problem()
    g = level0_geom(pr, lib)
    lay = lib.Layout.decompose(tuple(pr["n"]), pr["max_grid_size"], nranks)
    ns = N.NavierStokes(g, lay, N.ns_params(**pr["params"]), solver_opts(pr, lib))
    init_level(ns, lay, lib, N, pr, pr["n"])
    return ns, lay, g, pr


def level_arrays(ns, lay, N, derived=()):
    """valid-region arrays of the boxes of the level THIS RANK owns (local_indices(lay) says which of lay.boxes they are): the state
    components, then the derived quantities asked for (NavierStokes::derive -- collective: its ghost fill talks to the other ranks, so
    every rank calls this, also one that owns nothing)"""
    import numpy as np
    S = ns.data(N.NavierStokes.S_NEW)
    # the six names of "velocity_average" (plotfile.plot_selection) are ONE derived quantity of six components; all the others are formed
    # by ONE derive_fields call (the velocity-gradient names among them share one ghost fill and one launch)
    va = N.NavierStokes.VEL_AVG_NAMES
    single = [name for name in derived if name not in va]
    D = ([ns.derive(single)] if single else []) + ([ns.derive("velocity_average")] if va[0] in derived else [])
    order = [(single + va).index(name) for name in derived]
    boxes, arrs = [], []
    for li in range(S.nlocal()):
        a, lo = S.to_numpy(li)
        blo, bhi, gi = lay.local_box(li)
        ng = (a.shape[0] - (bhi[0] - blo[0] + 1)) // 2
        v = a[ng:a.shape[0] - ng, ng:a.shape[1] - ng, ng:a.shape[2] - ng, :]
        arrs.append(np.concatenate([v, np.concatenate([d.to_numpy(li)[0] for d in D], axis=-1)[..., order]], axis=-1) if D else v.copy())
        boxes.append((tuple(blo), tuple(bhi)))
    return boxes, arrs


def plot_names_and_filter(pr):
    """(names of everything level_arrays returns for this run, derived names, predicate name -> written?): amr.plot_vars picks among the
    state variables, amr.derive_plot_vars adds derived ones (plotfile.plot_selection)"""
    from .plotfile import state_names, plot_selection
    state = state_names(pr["params"].get("do_trac2", 0), pr["params"].get("do_temp", 0))
    pv = pr.get("plot_vars", "ALL")
    if pr.get("slab") and isinstance(pv, list):          # a 2-D inputs file names the plane's velocities x_velocity, y_velocity: y is the slab's z
        pv = ["z_velocity" if v == "y_velocity" else v for v in pv]
    keep, der = plot_selection(state, pv, pr.get("derive_plot_vars", "NONE"), averaging=pr["params"].get("avg_interval", 0) > 0,
                               particles=bool(pr.get("particles")))
    kept = {state[q] for q in keep} | set(der)
    return state + der, der, kept


def select_components(names, arrs, kept, renamed=None):
    """drop the components amr.plot_vars does not name; `renamed`: names after _plane's renaming, same order as `names`"""
    idx = [q for q, nm in enumerate(names) if nm in kept]
    out = renamed if renamed is not None else names
    return [out[q] for q in idx], [a[..., idx] for a in arrs]


def _plane(boxes, arrs, names):
    """the (x, z) plane of a 2-D run lifted onto a y-periodic slab (inputs.Inputs.lift_2d) as 2-D boxes / arrays / names: the boxes that
    start at y = 0, their first y-plane, the y-velocity (identically zero) dropped, z_velocity renamed"""
    import numpy as np
    from .plotfile import PARTICLE_DERIVE_NAMES
    keep = [q for q, (lo, hi) in enumerate(boxes) if lo[1] == 0]
    comps = [0, 2] + list(range(3, len(names)))
    # the particle counts are the one thing that varies across the slab (the particles sit in its middle): the plane holds their sum
    cnt = [q for q, nm in enumerate(names) if nm in PARTICLE_DERIVE_NAMES]
    flat = [q for q in range(len(names)) if q not in cnt]
    # what makes the slab a 2-D run: no variation across it, no flow along it (checked on everything written; enforce_plane keeps it so)
    for a in arrs:
        scale = max(1.0, float(np.abs(a[..., flat]).max()))
        dev = max(float(np.abs(a[..., flat] - a[:, :1][..., flat]).max()), float(np.abs(a[..., 1]).max()))
        if dev > 1e-8 * scale:
            raise RuntimeError(f"iamr_amd.run: the slab of a two-dimensional run lost its uniformity (deviation {dev:.3e}, scale {scale:.3e})")
    n2 = ["x_velocity", "y_velocity"] + list(names[3:])
    planes = []
    for q in keep:
        pl = arrs[q][:, 0, :, :].copy()
        if cnt:
            foot = lambda b: (b[0][0], b[0][2], b[1][0], b[1][2])
            pl[..., cnt] = sum(arrs[s][..., cnt].sum(axis=1) for s in range(len(boxes)) if foot(boxes[s]) == foot(boxes[q]))
        planes.append(pl[..., comps].copy())
    return ([((boxes[q][0][0], boxes[q][0][2]), (boxes[q][1][0], boxes[q][1][2])) for q in keep], planes, n2)


def sum_lines(time, sums, pr=None):
    """the three lines of NavierStokes::sum_integrated_quantities (NavierStokes.cpp:1075-1078; 12 significant digits) for (mass, tracer,
    kinetic energy).  A two-dimensional run on its slab reports the plane integrals: the sums divided by the slab's thickness."""
    if pr is not None and pr.get("slab"):
        thick = pr["prob_hi"][1] - pr["prob_lo"][1]
        sums = [v / thick for v in sums]
    return [f"TIME= {time:.12g} {name}= {v:.12g}" for name, v in zip(("MASS", "TRAC", "KINETIC ENERGY"), sums)]


def say_sums(say, time, sums, pr):
    say("")
    for line in sum_lines(time, sums, pr):
        say(line)


def take_profile(run, pr, step, rank, say):
    """ns.profile_interval > 0: every that many level-0 steps (and for the initial data, step 0) the plane-averaged profile of the level or
    the hierarchy (profile.py) goes to <ns.profile_file><step:05d>.  Collective: every rank takes part in the reduction, rank 0 writes.
    A bin level above the finest level of the moment is clamped to it (a regrid changes the finest level)."""
    pf = pr.get("profile") or {}
    if pf.get("interval", -1) <= 0 or step % pf["interval"] != 0:
        return
    from .profile import write_profile
    p = run.plane_profile(pf["dir"], min(pf["level"], run.nlev - 1))
    if rank == 0:
        path = f"{pf['file']}{step:05d}"
        write_profile(path, p, step, run.time)
        say("PROFILE:", path)


def take_spectrum(run, pr, step, rank, say):
    """ns.spectrum_interval > 0: every that many level-0 steps (and for the initial data, step 0) the shell-summed spectra of the level, or
    of level 0 of the hierarchy (spectrum.py), go to <ns.spectrum_file><step:05d>.  Collective: every rank takes part, rank 0 writes."""
    sp = pr.get("spectrum") or {}
    if sp.get("interval", -1) <= 0 or step % sp["interval"] != 0:
        return
    from .spectrum import write_spectrum
    s = run.spectrum()
    if rank == 0:
        path = f"{sp['file']}{step:05d}"
        write_spectrum(path, s, step, run.time)
        say("SPECTRUM:", path)


def take_plane_spectrum(run, pr, step, rank, say):
    """ns.plane_spectrum_interval > 0: every that many level-0 steps (and for the initial data, step 0) the ring-summed plane spectra of the
    level, or of level 0 of the hierarchy (planespec.py), along ns.plane_spectrum_dir go to <ns.plane_spectrum_file><step:05d>.
    Collective: every rank takes part, rank 0 writes.  Off: nothing is launched, allocated or printed."""
    ps = pr.get("plane_spectrum") or {}
    if ps.get("interval", 0) <= 0 or step % ps["interval"] != 0:
        return
    from .planespec import write_plane_spectrum
    s = run.plane_spectrum(ps["dir"])
    if rank == 0:
        path = f"{ps['file']}{step:05d}"
        write_plane_spectrum(path, s, step, run.time)
        say("PLANE SPECTRUM:", path)


def take_budget(run, pr, step, rank, say):
    """ns.budget_interval > 0: every that many level-0 steps (and for the initial data, step 0) the spectral kinetic-energy budget of the
    level, or of level 0 of the hierarchy (budget.py), goes to <ns.budget_file><step:05d>.  Collective: every rank takes part, rank 0
    writes.  Off: nothing is launched, allocated or printed."""
    bd = pr.get("budget") or {}
    if bd.get("interval", -1) <= 0 or step % bd["interval"] != 0:
        return
    from .budget import write_budget
    s = run.spectral_budget()
    if rank == 0:
        path = f"{bd['file']}{step:05d}"
        write_budget(path, s, step, run.time)
        say("BUDGET:", path)


def take_sgs(run, pr, step, rank, say):
    """ns.sgs_interval > 0: every that many level-0 steps (and for the initial data, step 0) the a-priori LES statistics of the level, or
    of level 0 of the hierarchy (sgs.py), go as one row per cut-off of ns.sgs_kc to the text file ns.sgs_file.  Collective: every rank
    takes part, rank 0 writes.  Off: nothing is launched or allocated."""
    sg = pr.get("sgs") or {}
    if sg.get("interval", -1) <= 0 or step % sg["interval"] != 0:
        return
    from .sgs import append_row
    for kc in sg["kc"]:
        s = run.sgs(sg["filter"], kc)
        if rank == 0:
            append_row(sg["file"], step, run.time, kc, s["stats"], (s["N"], s["negative_cells"]))


def take_strfn(run, pr, step, rank, say):
    """ns.strfn_interval > 0: every that many level-0 steps (and for the initial data, step 0) the structure functions and two-point
    correlations of the level, or of level 0 of the hierarchy (strfn.py), go to <ns.strfn_file><step:05d>.  Collective: every rank takes
    part, rank 0 writes.  Off: nothing is launched or allocated."""
    sf = pr.get("strfn") or {}
    if sf.get("interval", -1) <= 0 or step % sf["interval"] != 0:
        return
    from .strfn import write_strfn
    s = run.structure_functions(sf["pmax"], sf["rmax"])
    if rank == 0:
        path = f"{sf['file']}{step:05d}"
        write_strfn(path, s, step, run.time)
        say("STRFN:", path)


def take_pdf(run, pr, step, rank, say):
    """ns.pdf_interval > 0: every that many level-0 steps (and for the initial data, step 0) the histograms and PDFs of the fields of
    ns.pdf_vars over the level or the hierarchy (pdf.py) go to <ns.pdf_file><step:05d>.  Collective: every rank takes part, rank 0
    writes.  A two-dimensional file names the plane's velocities x_velocity, y_velocity (y is the slab's z); the slab is uniform across
    its thickness, so the normalised PDF is the plane's, the counts are those of slab cells."""
    pf = pr.get("pdf") or {}
    if pf.get("interval", -1) <= 0 or step % pf["interval"] != 0:
        return
    from .pdf import write_pdf
    names = ["z_velocity" if pr.get("slab") and v == "y_velocity" else v for v in pf["vars"]]
    h = run.histogram(names, pf["nbins"], pf["range"])
    h["names"] = tuple(pf["vars"])
    if rank == 0:
        path = f"{pf['file']}{step:05d}"
        write_pdf(path, h, step, run.time)
        say("PDF:", path)


def take_integrals(run, pr, step, rank, say):
    """ns.integrate_interval > 0: every that many level-0 steps (and for the initial data, step 0) the volume integrals of the fields of
    ns.integrate_vars over the level or the hierarchy go as one row `step time v1 ... vn` to the text file ns.integrate_file
    (integrals.py).  Collective: every rank takes part, rank 0 writes.  A two-dimensional run on its slab reports the plane integrals: the
    sums divided by the slab's thickness (as sum_lines does)."""
    ig = pr.get("integrate") or {}
    if ig.get("interval", 0) <= 0 or step % ig["interval"] != 0:
        return
    from .integrals import append_row
    v = run.integrate(ig["vars"])
    if pr.get("slab"):
        v = v / (pr["prob_hi"][1] - pr["prob_lo"][1])
    if rank == 0:
        append_row(ig["file"], ig["vars"], step, run.time, v)


def enforce_plane(levels, pr):
    """a two-dimensional run on its y-periodic slab (inputs.Inputs.lift_2d) after every coarse time step: the state, the pressure and its
    gradient become their means across the slab, the velocity / gradient component along it zero.  Upstream's 2-D build has no third
    direction to perturb; here the multigrid smoothers' (i + j + k) colouring leaves iteration error at the level of the solver
    tolerances that varies across the slab, which a flow that amplifies perturbations would grow into real three-dimensional motion over
    many steps.  Projecting it out each step keeps the run the 2-D run the inputs file describes (deviations removed are of the size of
    the solver tolerances; `_plane` still checks everything written).  Single-rank runs (every box is local)."""
    import numpy as np
    for l, lev in enumerate(levels):
        n = [v * 2 ** l for v in pr["n"]]
        for which, along in ((lev.S_NEW, 1), (lev.P_NEW, None), (lev.GP_NEW, 1)):
            mf = lev.data(which)
            G = mf.gather_valid(n)
            plane = G[:, :n[1]].mean(axis=1)                     # nodal in y: node n[1] is the periodic image of node 0
            if along is not None:
                plane[..., along] = 0.0
            for li in range(mf.nlocal()):
                a, lo = mf.to_numpy(li)
                blo, bhi, _ = mf.layout.local_box(li)
                vx = slice(blo[0] - lo[0], bhi[0] + mf.typ[0] - lo[0] + 1)
                vz = slice(blo[2] - lo[2], bhi[2] + mf.typ[2] - lo[2] + 1)
                vy = slice(blo[1] - lo[1], bhi[1] + mf.typ[1] - lo[1] + 1)
                a[vx, vy, vz] = plane[blo[0]:bhi[0] + mf.typ[0] + 1, None, blo[2]:bhi[2] + mf.typ[2] + 1]
                mf.from_numpy(a, li)
            lev.set_data(which, mf)


def setup_particles(run, pr, say, restart_dir=None):
    """tracer particles of a run with particles.* keys (NavierStokesBase::initParticleData / post_restart_particle,
    NavierStokesBase.cpp:3808-3864): one container for the level or the hierarchy; at start-up the positions of particles.particle_init_file;
    on a restart the checkpoint's Particles/ (unless particles.restart_from_nonparticle_chkfile), then particles.particle_restart_file is
    added and particles.particle_output_file written.  A two-dimensional file lifts (x, y) to (x, mid-slab, y) and the particles never move
    across the slab.  With particles.do_timestamps = 1 the timestamp directory is made and the container told to write its records
    there (<dir>/Timestamp_NN, appended to: a restart continues them).  Several ranks: every call below is collective; rank 0 passes a file's positions and the other ranks none (the ids are
    then those of a one-rank run), the checkpoint's particles are read in shares, and the PARTICLES: line speaks of all ranks.  Returns
    the container or None."""
    pp = pr.get("particles")
    if not pp:
        return None
    from .lib import comm_rank
    import numpy as np
    from . import particles as P
    rank = comm_rank()[0]
    from_file = lambda name: P.read_particle_file(name, slab_y) if rank == 0 else np.zeros((0, 3))
    pc = P.Particles.for_run(run)
    slab_y = None
    if pr.get("slab"):
        pc.set_fixed_dir(1)
        slab_y = 0.5 * (pr["prob_lo"][1] + pr["prob_hi"][1])
    run.set_particles(pc)
    ts = pp.get("timestamp")
    if ts:
        from .lib import comm_barrier
        if rank == 0:
            os.makedirs(ts["dir"], exist_ok=True)
        comm_barrier()                                  # the directory exists
        pc.set_timestamp(os.path.join(ts["dir"], "Timestamp"), ts["indices"])
        say(f"PARTICLES: timestamp records of state components {ts['indices']} go to {os.path.join(ts['dir'], 'Timestamp')}_NN")
    if restart_dir is None:
        if pp["init_file"]:
            pc.add(from_file(pp["init_file"]))
    else:
        if not pp["restart_from_nonparticle_chkfile"]:
            P.restore(restart_dir, pc)
        if pp["restart_file"]:
            pc.add(from_file(pp["restart_file"]))
        if pp["output_file"]:
            xyz, ids, cpus = P.gather_sorted(pc)
            if rank == 0:
                P.write_ascii(pp["output_file"], xyz, ids, cpus)
    if pp["verbose"]:
        say(f"PARTICLES: {pc.count_global()} (removed outside the domain: {pc.removed})")
    return pc


def plot_particles(run, pr, path):
    """particles.particles_in_plotfile (NavierStokes.cpp:1201-1205): the plotfile gets the Particles/ directory of a checkpoint"""
    pc = run.particles
    if pc is not None and pr["particles"]["in_plotfile"]:
        from .particles import save
        save(path, pc)
    return path


def write_plot(run, lay, pr, N, step, root):
    """NavierStokesBase::writePlotFile role: AMReX-format plotfile <root><step:05d> with every level of `run` (a level or a hierarchy): the
    state variables of amr.plot_vars and the derived quantities of amr.derive_plot_vars.  `lay`: the layouts of the levels (for a single
    level its layout will do); they name all boxes and their owners.  Collective: every rank of the library's communicator calls it and
    writes the boxes it owns (plotfile.write_collective).  A two-dimensional run (single-rank: every box is local) writes its plane."""
    from .plotfile import PlotFile, Level, write_collective
    from .lib import comm_rank
    rank, world = comm_rank()
    lays = lay if isinstance(lay, (list, tuple)) else [lay]
    names, der, kept = plot_names_and_filter(pr)
    slab = pr.get("slab")
    ax = [0, 2] if slab else [0, 1, 2]                      # the directions the plotfile knows
    levels = []
    for l, lev in enumerate(run.levels):
        n = [v * 2 ** l for v in pr["n"]]
        dx = [(pr["prob_hi"][d] - pr["prob_lo"][d]) / n[d] for d in range(3)]
        boxes, arrs = level_arrays(lev, lays[l], N, der)
        if slab:
            boxes, arrs, names2 = _plane(boxes, arrs, names)
            out_names, arrs = select_components([nm for q, nm in enumerate(names) if q != 1], arrs, kept, names2)
            owned = None
        else:
            out_names, arrs = select_components(names, arrs, kept)
            boxes, owned = lays[l].boxes, local_indices(lays[l])
        levels.append(Level(([0] * len(ax), [n[d] - 1 for d in ax]), [dx[d] for d in ax], boxes, arrs, step * 2 ** l, run.time, owned=owned))
    pf = PlotFile(out_names, run.time, [pr["prob_lo"][d] for d in ax], [pr["prob_hi"][d] for d in ax], levels)
    path = f"{root}{step:05d}"
    if slab:
        pf.write(path)
    else:
        write_collective(pf, path, [ll.owners for ll in lays], rank, world)
    return plot_particles(run, pr, path)


# ---- what a hierarchy and a single level do differently in the main loop
def _hierarchy(run):
    from .amr import Amr
    return isinstance(run, Amr)


def advance(run):
    """one coarse time step -> its dt"""
    return run.coarse_step() if _hierarchy(run) else run.step()


def step_line(run, step, dt):
    line = f"STEP = {step} TIME = {run.time:.12g} DT = {dt:.12g}"
    return line + f" LEVELS = {run.nlev} GRIDS = {[len(l.boxes) for l in run.layouts]}" if _hierarchy(run) else line


def report_sums(run, pr, step, say):
    """ns.sum_interval > 0: the integrated quantities of the initial data (step 0; NavierStokes.cpp:1284-1285) and of every sum_interval-th
    level-0 step (post_timestep, NavierStokesBase.cpp:2589-2592).  A hierarchy sums by itself and is asked for what it found; the
    driver of a single level sums when they are due."""
    if _hierarchy(run):
        ls = run.last_sum()
        if ls is not None and ls[0] == step:    # (a slab was flattened after the step: what is reported is what is kept)
            say_sums(say, ls[1], run.sum_integrated() if pr.get("slab") and step > 0 else ls[2], pr)
    elif pr["params"].get("sum_interval", -1) > 0 and step % pr["params"]["sum_interval"] == 0:
        say_sums(say, run.time, run.sum_integrated(), pr)


def take_time_average(run, pr, step, dt):
    """ns.avg_interval > 0: a hierarchy samples by itself; the driver of a single level after post_init (step 0, dt None: the level's dt;
    NavierStokes.cpp:1286-1297) and after every step (NavierStokesBase.cpp:2630-2634)"""
    if not _hierarchy(run) and pr["params"].get("avg_interval", 0) > 0:
        run.time_average(run.dt if dt is None else dt, step)


def drive(pr, inp, lib, N, hierarchy, rank=0, world=1, observe=None):
    """a run from amr.restart or from its initial data to max_step / stop_time: a single level, or (hierarchy) an Amr hierarchy.  world > 1:
    the boxes of every level are spread over the ranks (level 0 by Layout.decompose, fixed refined grids round-robin, regridded levels
    by the library's knapsack, restarted levels as checkpoint.restart says) and every rank executes the same sequence of collective
    operations: step, enforce_plane, sums, time average, profile, spectrum, plane spectrum, spectral budget, a-priori LES statistics, structure functions, pdf, integrals, observe, plotfile, checkpoint.  observe: see main"""
    from . import checkpoint
    say = print if rank == 0 else (lambda *a, **k: None)
    plot_int, plot_root = pr.get("plot_int", -1), pr.get("plot_file", "plt")
    check_int, check_root = pr.get("check_int", -1), pr.get("check_file", "chk")

    def post_step(step, dt):
        """NavierStokes::post_init for the initial data (step 0, dt None), post_timestep of level 0 after a step, and the output then due"""
        report_sums(run, pr, step, say)
        take_time_average(run, pr, step, dt)
        take_profile(run, pr, step, rank, say)
        take_spectrum(run, pr, step, rank, say)
        take_plane_spectrum(run, pr, step, rank, say)
        take_budget(run, pr, step, rank, say)
        take_sgs(run, pr, step, rank, say)
        take_strfn(run, pr, step, rank, say)
        take_pdf(run, pr, step, rank, say)
        take_integrals(run, pr, step, rank, say)
        if observe:
            observe(run, step, dt)
        if plot_int > 0 and step % plot_int == 0:           # collective: every rank writes, rank 0 reports
            say("PLOTFILE:", write_plot(run, run.layouts, pr, N, step, plot_root))

    ig = pr.get("integrate") or {}
    if ig.get("interval", 0) > 0 and rank == 0:
        # the one file of the run's integrals: started afresh (header line) by a run from initial data, appended to after amr.restart
        from .integrals import start_file
        start_file(ig["file"], ig["vars"], append=bool(pr.get("restart")))
    sg = pr.get("sgs") or {}
    if sg.get("interval", -1) > 0 and rank == 0:
        # the one file of the run's a-priori LES statistics, by the same rule
        from .sgs import start_file as start_sgs
        start_sgs(sg["file"], append=bool(pr.get("restart")))
    if pr.get("restart"):
        # amr.restart (Amr::restart): grids, data, times and step counters come from the checkpoint, parameters from the inputs file
        # (the solvers' options are the run's too: a two-dimensional run restarts with its slab multigrid, see solver_opts)
        run = checkpoint.restart(pr["restart"], level0_geom(pr, lib), N.ns_params(**pr["params"]), opts=solver_opts(pr, lib),
                                 single_level=not hierarchy, stop_time=pr["stop_time"], rank=rank, world=world)
        if pr.get("regrid"):
            run.set_regrid(**pr["regrid"])
        step = checkpoint.read_header(pr["restart"])["level_steps"][0]
        say(f"RESTART from {pr['restart']}: step {step}, time {run.time:.12g}" + (f", levels {run.nlev}" if hierarchy else ""))
        setup_particles(run, pr, say, pr["restart"])
    else:
        run = build_amr(pr, lib, N, world)[0] if hierarchy else build(inp, lib, N, world, pr)[0]
        run.post_init(pr["stop_time"])
        setup_particles(run, pr, say)               # (nothing moves them during the initial iterations: NavierStokes.cpp:672-677)
        step = 0
        post_step(0, None)
    if inp.ignored:
        say("inputs: ignored (I/O / verbosity / AMR bookkeeping) keys:", " ".join(sorted(inp.ignored)))
    t0 = time.perf_counter()
    while (pr["max_step"] < 0 or step < pr["max_step"]) and (pr["stop_time"] < 0 or run.time < pr["stop_time"] - 1e-14):
        if pr["max_step"] < 0 and pr["stop_time"] < 0:
            break
        dt = advance(run)
        if pr.get("slab"):
            enforce_plane(run.levels, pr)
        step += 1
        say(step_line(run, step, dt))
        post_step(step, dt)
        if check_int > 0 and step % check_int == 0:
            say("CHECKPOINT:", checkpoint.write(run, check_root, step, pr.get("max_level") if hierarchy else None))
    lib.sync()
    say(f"Run time = {time.perf_counter() - t0:.6f}")
    return 0


def main(argv, observe=None):
    """observe (optional): called as observe(run, step, dt) with the level or the hierarchy once the initial data are in place (step 0, dt
    None; not after a restart) and after every coarse step -- for callers that follow a run from inside its own loop"""
    from .inputs import Inputs
    files = [a for a in argv if "=" not in a]
    over = [a for a in argv if "=" in a]
    if not files:
        print(__doc__)
        return 2
    inp = Inputs(files, over)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    from . import comm, lib
    from . import ns as N
    # IAMRX_RUN_TRANSPORT=gloo: host-staged transport, every rank on device 0 -- several ranks on one GPU, where RCCL cannot connect two
    # ranks; unset: nccl + RCCL, rank r on GPU LOCAL_RANK.  IAMRX_RUN_TIMEOUT (seconds; unset: torch's default): how long a collective
    # waits for a rank that never calls it
    timeout_s = float(os.environ["IAMRX_RUN_TIMEOUT"]) if os.environ.get("IAMRX_RUN_TIMEOUT") else None
    comm.start(rank, world, local_rank, os.environ.get("IAMRX_RUN_TRANSPORT", ""), timeout_s)
    pr = inp.problem()
    if pr.get("slab") and world > 1:
        raise NotImplementedError("iamr_amd.run: two-dimensional inputs (run on a y-periodic slab) are single-rank runs")
    hierarchy = bool(pr["fine_boxes"] or pr.get("regrid") or (pr.get("restart") and pr.get("max_level", 0) > 0))
    if pr.get("spectral_distributed"):          # before the first spectrum or budget: they take the slab-decomposed transform on several ranks
        lib.tuning_set("SPECTRUM_DIST", 1)
    rc = drive(pr, inp, lib, N, hierarchy, rank, world, observe)
    comm.stop()
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

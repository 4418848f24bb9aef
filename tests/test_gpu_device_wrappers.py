"""The device-resident wrappers of the fused likelihood (device.loglik*_device) against driver.loglik, which reaches the same
kernels through the host-buffer entry points: one marshaller builds every trpl_loglik*_dev call (device._loglik_dev), so an
argument in the wrong slot shows as a different bit somewhere.  Same tiny problem as tests/test_loglik_marshal_host.py --
S = 5, C = 2 films of different thickness, L = 32, T = 96, 97 and 40 observations -- with the one-system stepper pinned on
both sides: every output is the host call's, bit for bit.  trpl_loglik_dev is the on-grid call and trpl_loglik_obs_dev the
off-grid one by construction; the three sinks take both.  Then the three passes over a resident PL block
(device.loglik*_from_pl_device) against each other."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S, C, L, T, TIME = 5, 2, 32, 96, 2.4
N_OBS = (97, 40)
OBS_LD = 97


@pytest.fixture(scope="module")
def problem(gpu, oracle):
    """Inputs, and the plain host-buffer run on and off the grid (the cut level comes from it)."""
    w = gpu.workloads
    rng = np.random.default_rng(29)
    ini, lens = w.twothick(L)
    ini, lens = np.ascontiguousarray(ini[:C]), np.ascontiguousarray(lens[:C])
    assert lens[0] != lens[1]
    X = w.samples(S, seed=13)
    sim_t = np.linspace(0, TIME, T + 1)
    mark = (w.MARKED_POINT * gpu.UNIT_CONVERSIONS)[None, :-1]
    lg = [np.log10(oracle.pvsim(mark, lens[c], TIME, L, T, ini[c])["plI"][0]) for c in range(C)]
    times = [rng.uniform(0.0, TIME, n) for n in N_OBS]                              # unsorted, off the grid
    obs = {False: [lg[c][:n] + rng.normal(0, 0.05, n) for c, n in enumerate(N_OBS)],
           True: [np.interp(times[c], sim_t, lg[c]) + rng.normal(0, 0.05, n) for c, n in enumerate(N_OBS)]}
    weights = [rng.uniform(0.1, 3.0, n) for n in N_OBS]
    plain = {}
    for off in (False, True):
        info = {}
        P = gpu.loglik(X, ini, lens, TIME, L, T, obs[off], kernel="single", info=info, times=times if off else None)
        assert not info["status"].any()
        plain[off] = dict(info, P=P)
    return dict(X=X, ini=ini, lens=lens, sim_t=sim_t, times=times, obs=obs, weights=weights, plain=plain)


def _padded(rows, fill, dtype=np.float64):
    m = np.full((C, OBS_LD), fill, dtype=dtype)
    for c, r in enumerate(rows):
        m[c, :len(r)] = r
    return m


def _staged(gpu, p, off):
    """The device tensors of one call: observations and weights sorted by time and padded as driver.loglik stages them."""
    import torch
    order = [np.argsort(t, kind="stable") for t in p["times"]] if off else [np.arange(n) for n in N_OBS]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = dict(X=dev(p["X"]), ini=dev(p["ini"]), obs=dev(_padded([o[i] for o, i in zip(p["obs"][off], order)], 0.0)),
             wts=dev(_padded([w[i] for w, i in zip(p["weights"], order)], 0.0)), br={})
    if off:
        br = [gpu.bracket_times(p["sim_t"], t[i]) for t, i in zip(p["times"], order)]
        d["br"] = dict(obs_hi=dev(_padded([b[0] for b in br], 1, np.int32)), obs_dx=dev(_padded([b[1] for b in br], 0.0)),
                       obs_h=dev(_padded([b[2] for b in br], 1.0)))
    return d


CASES = [("plain", False), ("plain", True), ("moments", False), ("moments", True), ("cut", False), ("cut", True),
         ("weighted", False), ("weighted", True)]


@pytest.mark.parametrize("sink,off", CASES, ids=["%s-%s" % (s, "times" if o else "grid") for s, o in CASES])
def test_device_wrapper_equals_the_host_buffer_call_bit_for_bit(gpu, problem, sink, off):
    import torch
    D, p = gpu.device, problem
    d = _staged(gpu, p, off)
    flags = gpu._abi.kernel_flag("single")
    P = torch.zeros(S, dtype=torch.float64, device="cuda")
    sse, esum = (torch.zeros((C, S), dtype=torch.float64, device="cuda") for _ in range(2))
    st, fl, cc = (torch.full((C, S), 7, dtype=torch.int32, device="cuda") for _ in range(3))
    it = torch.zeros((C, S), dtype=torch.int64, device="cuda")
    common = (d["X"], d["ini"], p["lens"], TIME, L, T, d["obs"])
    opt = dict(status=st, iters_total=it, flags=flags, floor_col=fl)
    host_kw = dict(kernel="single", times=p["times"] if off else None)
    info = {}
    if sink == "plain":
        want = p["plain"][off]
        if off:
            D.loglik_obs_device(*common, d["br"]["obs_hi"], d["br"]["obs_dx"], d["br"]["obs_h"], N_OBS, P, sse, **opt)
        else:
            D.loglik_device(*common, N_OBS, P, sse, **opt)
        got = dict(P=P, sse=sse)
    elif sink == "moments":
        gpu.loglik(p["X"], p["ini"], p["lens"], TIME, L, T, p["obs"][off], info=info, mag_profile=True, **host_kw)
        want = info
        D.loglik_moments_device(*common, N_OBS, P, sse, esum, **opt, **d["br"])
        got = dict(P=P, sse=sse, esum=esum)
    elif sink == "weighted":
        gpu.loglik(p["X"], p["ini"], p["lens"], TIME, L, T, p["obs"][off], info=info, weights=p["weights"], **host_kw)
        want = info
        D.loglik_weighted_device(*common, d["wts"], N_OBS, P, sse, esum, **opt, **d["br"])
        got = dict(P=P, sse=sse, esum=esum)
    else:
        level = float(np.median(p["plain"][off]["sse"].sum(axis=0)))
        Ph = gpu.loglik(p["X"], p["ini"], p["lens"], TIME, L, T, p["obs"][off], info=info, sse_cut=level, **host_kw)
        want = dict(info, P=Ph)
        assert (want["cut_col"] >= 0).any() and (want["cut_col"] == -1).any()          # some systems cut, some not
        D.loglik_cut_device(*common, N_OBS, level, P, sse, cut_col=cc, **opt, **d["br"])
        got = dict(P=P, sse=sse, cut_col=cc)
    torch.cuda.synchronize()
    got.update(status=st, iters_total=it, floor_col=fl)
    assert np.isfinite(want["P"]).all() and (want["sse"] > 0).all()
    for k, t in got.items():
        assert np.array_equal(t.cpu().numpy(), want[k]), (sink, off, k)


@pytest.fixture(scope="module")
def pl_block(gpu, problem):
    """Curve 0's PL of the S samples, solved once into HBM."""
    import torch
    p = problem
    pl = torch.empty((S, T + 1), dtype=torch.float64, device="cuda")
    st = torch.zeros(S, dtype=torch.int32, device="cuda")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    gpu.device.solve_pl_device(dev(p["X"][:, :12]), p["lens"][0], TIME, L, T, dev(p["ini"][0]), pl, status=st,
                               flags=gpu._abi.kernel_flag("single"))
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any()
    return pl, st, dev(p["X"][:, 12])


@pytest.mark.parametrize("off", [False, True], ids=["grid", "times"])
def test_the_three_passes_over_a_resident_pl_block_agree(gpu, problem, pl_block, off):
    import torch
    D, p = gpu.device, problem
    pl, st, mag = pl_block
    d = _staged(gpu, p, off)
    obs = d["obs"][0].contiguous()
    br = {k: v[0].contiguous() for k, v in d["br"].items()}
    new = lambda: torch.zeros(S, dtype=torch.float64, device="cuda")
    out = {name: dict(P=new(), sse=new()) for name in ("plain", "moments", "ones")}
    D.loglik_from_pl_device(pl, obs, mag, status=st, **out["plain"], **br)
    for name in ("moments", "ones"):
        out[name]["esum"] = new()
    D.loglik_moments_from_pl_device(pl, obs, mag, status=st, **out["moments"], **br)
    D.loglik_weighted_from_pl_device(pl, obs, torch.ones_like(obs), mag, status=st, **out["ones"], **br)
    torch.cuda.synchronize()
    out = {name: {k: t.cpu().numpy() for k, t in o.items()} for name, o in out.items()}
    assert (out["plain"]["sse"] > 0).all() and np.isfinite(out["moments"]["esum"]).all() and out["moments"]["esum"].any()
    assert np.array_equal(out["moments"]["sse"], out["plain"]["sse"]) and np.array_equal(out["moments"]["P"], out["plain"]["P"])
    for k in ("P", "sse", "esum"):
        assert np.array_equal(out["ones"][k], out["moments"][k]), k


ENTRY = {("plain", False): "trpl_loglik", ("plain", True): "trpl_loglik_obs", "moments": "trpl_loglik_moments",
         "weighted": "trpl_loglik_weighted", "cut": "trpl_loglik_cut"}


def _raw(gpu, entry, at, d, lens, level, P, sse, esum, cut_col, status, iters, floor_col, tail, S_=S):
    """One call of a fused entry point, host-buffer or _dev, argument by argument as include/trpl.h lists them; `at` turns a
    buffer (or None) into its address, `tail` is (device, seconds) or (stream,)."""
    a = gpu._abi
    base = entry[:-4] if entry.endswith("_dev") else entry
    n_obs = np.array(N_OBS, dtype=np.int64)
    args = [at(d["X"]), S_, C, a.ptr(lens), TIME, L, T]
    if base != "trpl_loglik_obs":
        args.append(1)
    args += [7, 10000, at(d["ini"]), at(d["obs"])]
    if base == "trpl_loglik_weighted":
        args.append(at(d["wts"]))
    if base != "trpl_loglik":
        args += [at(d["br"].get(k)) for k in ("obs_hi", "obs_dx", "obs_h")]
    args += [OBS_LD, a.ptr(n_obs)]
    if base == "trpl_loglik_cut":
        args.append(float(level))
    args += [at(P), at(sse)]
    if base in ("trpl_loglik_moments", "trpl_loglik_weighted"):
        args.append(at(esum))
    if base == "trpl_loglik_cut":
        args.append(at(cut_col))
    args += [at(status), at(iters), at(floor_col), a.kernel_flag("single"), *tail]
    a.check(getattr(a.lib(), entry)(*args))


@pytest.mark.parametrize("sink,off", CASES, ids=["%s-%s" % (s, "times" if o else "grid") for s, o in CASES])
def test_host_buffer_forms_equal_their_device_forms_with_and_without_the_optional_outputs(gpu, problem, sink, off):
    """The five host-buffer entry points called directly, once with every optional output given and once with all of them NULL
    (sse, status, iters_total, floor_col, cut_col; esum is not optional where there is one): P, and esum, are the same either way,
    and every output given is the _dev form's bit for bit.  seconds is a clock: finite and > 0; 0 when there are no samples."""
    import ctypes
    import torch
    p = problem
    d = _staged(gpu, p, off)
    h = {k: (v.cpu().numpy() if k != "br" else {n: t.cpu().numpy() for n, t in v.items()}) for k, v in d.items()}
    entry = ENTRY.get((sink, off)) or ENTRY[sink]
    level = float(np.median(p["plain"][off]["sse"].sum(axis=0)))
    moments = sink in ("moments", "weighted")
    new = lambda dtype, fill, shape=(C, S): np.full(shape, fill, dtype=dtype)
    out = dict(P=new(np.float64, 0.0, (S,)), sse=new(np.float64, 0.0), esum=new(np.float64, 0.0) if moments else None,
               cut_col=new(np.int32, 7) if sink == "cut" else None, status=new(np.int32, 7), iters=new(np.int64, 0),
               floor_col=new(np.int32, 7))
    dev = {k: None if v is None else torch.from_numpy(v.copy()).cuda() for k, v in out.items()}
    sec = ctypes.c_double(-1.0)
    _raw(gpu, entry, gpu._abi.ptr, h, p["lens"], level, tail=(0, ctypes.byref(sec)), **out)
    _raw(gpu, entry + "_dev", lambda t: None if t is None else t.data_ptr(), d, p["lens"], level,
         tail=(torch.cuda.current_stream().cuda_stream,), **dev)
    torch.cuda.synchronize()
    assert np.isfinite(sec.value) and sec.value > 0
    assert np.isfinite(out["P"]).all() and (out["sse"] > 0).all() and (out["iters"] > 0).all() and (out["status"] != 7).all()
    for k, v in out.items():
        if v is not None:
            assert np.array_equal(v, dev[k].cpu().numpy()), (sink, off, k)
    bare = dict.fromkeys(out, None)
    bare.update(P=new(np.float64, 0.0, (S,)), esum=new(np.float64, 0.0) if moments else None)
    sec = ctypes.c_double(-1.0)
    _raw(gpu, entry, gpu._abi.ptr, h, p["lens"], level, tail=(0, ctypes.byref(sec)), **bare)
    assert np.isfinite(sec.value) and sec.value > 0
    assert np.array_equal(bare["P"], out["P"]) and (not moments or np.array_equal(bare["esum"], out["esum"]))
    sec = ctypes.c_double(-1.0)
    _raw(gpu, entry, gpu._abi.ptr, h, p["lens"], level, tail=(0, ctypes.byref(sec)), S_=0, **bare)
    assert sec.value == 0.0

"""The Python binding's call transcript: which C entry points a Python call reaches, in which order
and with which arguments, taken on a fake library so that no device is needed. Shared by
scripts/record_binding_transcript.py, which wrote tests/golden/binding_transcript.json.gz on the commit
before the engine classes got one base, and tests/test_binding_transcript_cpu.py, which replays the
same cases on the tree under test and only ever reads that file."""
import ctypes as C
import gc
import inspect
import sys

import numpy as np

import nlsolver_amd as N
from nlsolver_amd import _capi, tinyqr

ENGINE_CLASSES = ("DEEngine", "DERefEngine", "DEBatchEngine", "PSOEngine", "PSOBatchEngine", "BFGSEngine",
                  "LMEngine", "NMEngine", "NMPSOEngine", "SANNEngine")
MODULES = ("de", "pso", "nm", "nmpso", "sann", "lm", "bfgs")


# ---- the fake library ------------------------------------------------------------------------
def _struct(obj):
    """{type name: the fields' values in the order the C side reads them}"""
    out = []
    for name, typ in obj._fields_:
        v = getattr(obj, name)
        if typ is C.c_char_p:
            v = "null" if v is None else v.decode()
        elif typ is C.c_void_p:
            v = "null" if v is None else v
        out.append(v)
    return {type(obj).__name__: out}


def normalise(a):
    if a is None:
        return "null"
    if isinstance(a, (bool, np.bool_)):
        return int(a)
    if isinstance(a, (int, float)):
        return a
    if isinstance(a, np.integer):
        return int(a)
    if isinstance(a, np.floating):
        return float(a)
    if isinstance(a, bytes):
        from nlsolver_amd.de import rtc_library_path
        # (wherever this machine keeps hiprtc, or "" where it has none)
        return "rtc_library_path()" if a == rtc_library_path().encode() else a.decode()
    if isinstance(a, C.c_void_p):  # a handle
        return "null" if a.value is None else a.value
    if isinstance(a, C.Array):
        return f"{a._type_.__name__}[{len(a)}]"
    if isinstance(a, C._Pointer):
        return "ptr"
    obj = getattr(a, "_obj", None)  # byref(obj)
    if isinstance(obj, C.Structure):
        return _struct(obj)
    if obj is not None:
        return type(obj).__name__
    raise TypeError(f"no normal form for {a!r}")


class FakeLibrary:
    """Stands in for _capi._lib. Every symbol of _capi.SYMBOLS answers with a recorder, except those
    in `missing` (AttributeError: a library built without them); those in `fail` return 2."""

    def __init__(self, missing=(), fail=()):
        self.calls, self.missing, self.fail, self.created = [], set(missing), set(fail), 0

    def __getattr__(self, name):
        if name not in _capi.SYMBOLS or name in self.missing:
            raise AttributeError(name)

        def recorder(*args):
            self.calls.append([name] + [normalise(a) for a in args])
            if name == "nlsg_last_error":
                return b"fake"
            if name in self.fail:
                return 2
            if name.endswith("_lds_bytes"):
                return 1024
            if name == "nlsg_sann_chains_per_wave":
                return 1
            if name.endswith("_record_doubles"):
                return 8
            if "_create" in name:
                args[-1]._obj.value = 0x1000 + self.created
                self.created += 1
            if name == "nlsg_de_ref_log":  # one logged evaluation, so that the rows are fetched too
                args[-1]._obj.value = 1
            return 0

        return recorder


# ---- running one case ------------------------------------------------------------------------
def summary(r, inputs=()):
    """the shape of a return value: what kind of thing, how large, and whether it is the caller's memory"""
    if r is None:
        return "null"
    if isinstance(r, np.ndarray):
        own = any(np.shares_memory(r, i) for i in inputs)
        return f"ndarray{list(r.shape)}:{r.dtype}" + (":input" if own else "")
    if isinstance(r, (tuple, list)):
        return [summary(v, inputs) for v in r]
    if isinstance(r, _capi.Status):
        return "Status"
    if isinstance(r, (bool, int, float, str)):
        return r
    return type(r).__name__


def call(fn, *args, **kw):
    """fn(*args, **kw) -> summary of what it returns against the arrays it was given"""
    with np.errstate(all="ignore"):
        r = fn(*args, **kw)
    return summary(r, [a for a in list(args) + list(kw.values()) if isinstance(a, np.ndarray)])


class Case:
    def __init__(self, id, fn, missing=(), fail=()):
        self.id, self.fn, self.missing, self.fail = id, fn, tuple(missing), tuple(fail)


def record(case, fake):
    """Runs the case with `fake` already standing in _capi._lib: {"calls", "result", "error",
    "unraisable"} — what reached the library, what came back, what was raised, and what a __del__
    raised."""
    unraisable, hook = [], sys.unraisablehook
    sys.unraisablehook = lambda u: unraisable.append(repr(u.exc_value))
    result = error = None
    try:
        try:
            result = case.fn(fake)
        except Exception as e:  # noqa: BLE001 - the transcript is what was raised
            error = {"type": type(e).__name__, "code": getattr(e, "code", None), "text": str(e)}
            del e
    finally:
        sys.unraisablehook = hook
    return {"calls": fake.calls, "result": result, "error": error, "unraisable": unraisable}


# ---- what the cases build ----------------------------------------------------------------------
def C0():
    return N.CustomObjective("return xi * xi;")


def C2():
    return N.CustomObjective("double r = xi - p(0); return p(1) * r * r;", n_params=2)


def CVEC():
    return N.CustomObjective("return x.sum([&](double v, uint64_t) { return v * v; });", vector=True,
                             finish_body="return s / D;")


def CGRAD(n_params=0):
    return N.CustomObjective("return xi * xi;", grad_body="return 2.0 * xi;", n_params=n_params)


OBJECTIVES = {"name": lambda: "sphere", "id": lambda: 2, "custom0": C0, "custom2": C2, "vector": CVEC}

# class -> (arguments after the objective, keywords): batch 2, dim 2, pop 4
SHAPE = {"DEEngine": ((4, 2), {}), "DERefEngine": ((2, 4, 2), {}), "DEBatchEngine": ((2, 4, 2), {}),
         "PSOEngine": ((4, 2), {}), "PSOBatchEngine": ((2, 4, 2), {}), "BFGSEngine": ((2,), {"dim": 2}),
         "LMEngine": ((), {"batch": 2, "n": 2}), "NMEngine": ((2, 2), {}), "NMPSOEngine": ((2, 2), {}),
         "SANNEngine": ((2, 2), {})}


def make(cls, objective, **kw):
    args, shape = SHAPE[cls]
    return getattr(N, cls)(objective, *args, **{**shape, **kw})


HAS_SET_PARAMS = ("DEBatchEngine", "PSOBatchEngine", "BFGSEngine", "LMEngine", "NMEngine", "NMPSOEngine",
                  "SANNEngine")


def quad():
    return N.QuadDiagRank1(np.array([1.0, 2.0]), np.array([0.5, -0.5]), 0.25)


def tanh_model():
    return N.TanhRegression(np.full((2, 3, 2), 0.25), np.full((2, 3), 0.5))


def link_model():
    return N.LinkRegression.logistic(np.full((2, 3, 2), 0.25), np.full((2, 3), 0.5))


def curve_model():
    return N.CurveModel.exp_decay(np.linspace(0.0, 1.0, 8).reshape(2, 4), np.full((2, 4), 0.5))


def X():
    return np.full((2, 2), 0.5)


def ROWS():
    return np.array([[1.0, 2.0], [3.0, 4.0]])


SEEDS = [3, 2**64 + 5]  # the second wraps to 5
STATES = [[1, 2], [3, 4]]


def _built(cls, objective="name", **kw):
    """an engine of the class, and the fake's record cleared of its construction"""
    def build(fake):
        eng = make(cls, OBJECTIVES[objective](), **kw)
        fake.calls.clear()
        return eng
    return build


def _methods():
    """(id, engine maker, what to call on it) for every public method of every engine class"""
    P = 0x2000  # a device pointer, as dist.py hands them over
    uid = bytes(range(128))
    out = []

    def add(cls, name, fn, objective="name", **kw):
        out.append((f"{cls}.{name}", _built(cls, objective, **kw), fn))

    c = "DEEngine"
    add(c, "init", lambda e: call(e.init, np.full(2, 0.5)))
    add(c, "init:wrong-shape", lambda e: call(e.init, np.full(3, 0.5)))
    add(c, "step", lambda e: [call(e.step), call(e.step, 3)])
    add(c, "status", lambda e: call(e.status))
    add(c, "best", lambda e: call(e.best))
    add(c, "download", lambda e: [call(e.download), call(e.download, trace=True)])
    add(c, "download:shard", lambda e: call(e.download), shard_lo=1, shard_n=2)
    add(c, "upload", lambda e: call(e.upload, np.full((4, 2), 0.5), np.zeros(4)))
    add(c, "bound_counts", lambda e: call(e.bound_counts))
    add(c, "bound_state", lambda e: call(e.bound_state))
    add(c, "screen_counts", lambda e: call(e.screen_counts))
    add(c, "screen_state", lambda e: call(e.screen_state))
    add(c, "minimize", lambda e: [call(e.minimize, np.full(2, 0.5)), call(e.minimize, np.full(2, 0.5), 5)])
    add(c, "time_generation_kernel", lambda e: call(e.time_generation_kernel, 2))
    add(c, "time_turns", lambda e: call(e.time_turns, 2))
    add(c, "record_doubles", lambda e: call(e.record_doubles))
    add(c, "turn_begin", lambda e: call(e.turn_begin, P))
    add(c, "turn_end", lambda e: call(e.turn_end, P, 2))
    add(c, "turn_finalize", lambda e: call(e.turn_finalize, P, 2))
    add(c, "turn_generation", lambda e: call(e.turn_generation))
    add(c, "can_speculate", lambda e: call(e.can_speculate))
    add(c, "comm_attach", lambda e: call(e.comm_attach, uid, 2, 1))
    add(c, "step_sharded", lambda e: [call(e.step_sharded), call(e.step_sharded, 3)])
    add(c, "comm_ranks", lambda e: call(e.comm_ranks))

    c = "DERefEngine"
    add(c, "minimize", lambda e: call(e.minimize, X(), np.array(STATES, dtype=np.uint64)))
    add(c, "log", lambda e: call(e.log, 1), log_capacity=2)
    add(c, "log:no-capacity", lambda e: call(e.log, 1))
    add(c, "time_solve", lambda e: [call(e.time_solve, X(), STATES), call(e.time_solve, X(), STATES, 3)])

    c = "DEBatchEngine"
    add(c, "init", lambda e: call(e.init, X(), SEEDS))
    add(c, "step", lambda e: [call(e.step), call(e.step, 3)])
    add(c, "status", lambda e: call(e.status))
    add(c, "best", lambda e: call(e.best))
    add(c, "download", lambda e: call(e.download, 1))
    add(c, "upload", lambda e: call(e.upload, np.zeros((2, 4, 2)), np.zeros((2, 4))))
    add(c, "minimize", lambda e: call(e.minimize, X(), np.array(SEEDS[:1] * 2, dtype=np.uint64)))
    add(c, "minimize:params", lambda e: call(e.minimize, X(), SEEDS, params=ROWS()), "custom2")
    add(c, "minimize:params-without", lambda e: call(e.minimize, X(), SEEDS, params=ROWS()))
    add(c, "time_solve", lambda e: [call(e.time_solve, X(), SEEDS), call(e.time_solve, X(), SEEDS, 3)])
    add(c, "time_solve:params", lambda e: call(e.time_solve, X(), SEEDS, 2, params=ROWS()), "custom2")

    c = "PSOEngine"
    lo, hi = np.full(2, -1.0), np.full(2, 1.0)
    add(c, "init", lambda e: [call(e.init, lo, hi), call(e.init, -2.0, 2.0)])
    add(c, "step", lambda e: [call(e.step), call(e.step, 3)])
    add(c, "status", lambda e: call(e.status))
    add(c, "best", lambda e: call(e.best))
    add(c, "download", lambda e: call(e.download))
    add(c, "download:accelerated", lambda e: call(e.download), type=N.PSO_ACCELERATED, shard_lo=1, shard_n=2)
    add(c, "minimize", lambda e: [call(e.minimize, np.full(2, 0.5), lo, hi),
                                  call(e.minimize, np.full(2, 0.5), -1.0, 1.0, 5)])
    add(c, "time_move_kernel", lambda e: call(e.time_move_kernel, 2))
    add(c, "record_doubles", lambda e: call(e.record_doubles))
    add(c, "turn_begin", lambda e: call(e.turn_begin, P))
    add(c, "turn_end", lambda e: call(e.turn_end, P, 2))
    add(c, "comm_attach", lambda e: call(e.comm_attach, uid, 2, 1))
    add(c, "step_sharded", lambda e: [call(e.step_sharded), call(e.step_sharded, 3)])
    add(c, "comm_ranks", lambda e: call(e.comm_ranks))

    c = "PSOBatchEngine"
    add(c, "init", lambda e: [call(e.init, -X(), X(), SEEDS), call(e.init, -1.0, lo + 2, SEEDS)])
    add(c, "step", lambda e: [call(e.step), call(e.step, 3)])
    add(c, "status", lambda e: call(e.status))
    add(c, "best", lambda e: call(e.best))
    add(c, "download", lambda e: call(e.download, 1))
    add(c, "download:accelerated", lambda e: call(e.download, 1), type=N.PSO_ACCELERATED)
    add(c, "minimize", lambda e: call(e.minimize, -X(), X(), SEEDS))
    add(c, "minimize:params", lambda e: call(e.minimize, -X(), X(), SEEDS, params=ROWS()), "custom2")
    add(c, "minimize:params-without", lambda e: call(e.minimize, -X(), X(), SEEDS, params=ROWS()))
    add(c, "time_solve", lambda e: [call(e.time_solve, -X(), X(), SEEDS), call(e.time_solve, -1.0, 1.0, SEEDS, 3)])
    add(c, "time_solve:params", lambda e: call(e.time_solve, -X(), X(), SEEDS, 2, params=ROWS()), "custom2")

    c = "BFGSEngine"
    add(c, "init", lambda e: call(e.init, X()))
    add(c, "step", lambda e: [call(e.step), call(e.step, 3)])
    add(c, "unfinished", lambda e: call(e.unfinished))
    add(c, "identity_count", lambda e: call(e.identity_count))
    add(c, "download", lambda e: call(e.download))
    add(c, "download_state", lambda e: [call(e.download_state), call(e.download_state, hessian=False)])
    add(c, "minimize", lambda e: [call(e.minimize, X()), call(e.minimize, [[1, 2], [3, 4]])])
    add(c, "minimize:params", lambda e: call(e.minimize, X(), params=ROWS()), "custom2")
    add(c, "minimize:params-without", lambda e: call(e.minimize, X(), params=ROWS()))
    add(c, "hessian_bytes_per_iteration", lambda e: call(e.hessian_bytes_per_iteration))
    add(c, "hessian_bytes_per_iteration:symmetric", lambda e: call(e.hessian_bytes_per_iteration),
        symmetric=True, dim=300)
    add(c, "time_steps", lambda e: call(e.time_steps, 2))

    c = "LMEngine"
    add(c, "set_solver", lambda e: [call(e.set_solver, N._capi.LM_QR), e.cfg.solver])
    add(c, "minimize", lambda e: [call(e.minimize, X()), call(e.minimize, [[1, 2], [3, 4]])])
    add(c, "minimize:params", lambda e: call(e.minimize, X(), params=ROWS()), "custom2")
    add(c, "minimize:params-without", lambda e: call(e.minimize, X(), params=ROWS()))
    add(c, "covariance", lambda e: [call(e.covariance, X()), call(e.covariance, X(), "absolute"),
                                    call(e.covariance, X(), scale=N._capi.LM_COV_RESIDUAL)])
    add(c, "covariance:wrong-shape", lambda e: call(e.covariance, np.zeros((2, 3))))
    add(c, "covariance:wrong-scale", lambda e: call(e.covariance, X(), "relative"))
    add(c, "stderr", lambda e: [call(e.stderr, X()), call(e.stderr, X(), "absolute")])
    add(c, "time_solve", lambda e: [call(e.time_solve, X()), call(e.time_solve, X(), 3)])
    add(c, "time_solve:params", lambda e: call(e.time_solve, X(), 2, params=ROWS()), "custom2")
    add(c, "time_eval_kernel", lambda e: [call(e.time_eval_kernel, X()), call(e.time_eval_kernel, X(), 3)])
    add(c, "time_qr_kernel", lambda e: [call(e.time_qr_kernel, X()), call(e.time_qr_kernel, X(), 3)])

    c = "NMEngine"
    add(c, "minimize", lambda e: [call(e.minimize, X()), call(e.minimize, [[1, 2], [3, 4]])])
    add(c, "minimize:bounded", lambda e: [call(e.minimize, X(), hi, lo), call(e.minimize, X(), upper=1.0, lower=-1.0)],
        bounded=True)
    add(c, "minimize:params", lambda e: call(e.minimize, X(), params=ROWS()), "custom2")
    add(c, "minimize:params-without", lambda e: call(e.minimize, X(), params=ROWS()))
    add(c, "phase_cycles", lambda e: call(e.phase_cycles, X()))
    add(c, "time_solve", lambda e: [call(e.time_solve, X()), call(e.time_solve, X(), 3)])
    add(c, "time_solve:params", lambda e: call(e.time_solve, X(), 2, params=ROWS()), "custom2")

    c = "NMPSOEngine"
    add(c, "minimize", lambda e: [call(e.minimize, X()), call(e.minimize, [[1, 2], [3, 4]])])
    add(c, "minimize:bounded", lambda e: [call(e.minimize, X(), lo, hi), call(e.minimize, X(), lower=-1.0, upper=1.0)],
        bounded=True)
    add(c, "minimize:params", lambda e: call(e.minimize, X(), params=ROWS()), "custom2")
    add(c, "minimize:params-without", lambda e: call(e.minimize, X(), params=ROWS()))
    add(c, "time_solve", lambda e: [call(e.time_solve, X()), call(e.time_solve, X(), 3)])
    add(c, "time_solve:params", lambda e: call(e.time_solve, X(), 2, params=ROWS()), "custom2")

    c = "SANNEngine"
    add(c, "minimize", lambda e: [call(e.minimize, X()), call(e.minimize, [[1, 2], [3, 4]])])
    add(c, "minimize:params", lambda e: call(e.minimize, X(), params=ROWS()), "custom2")
    add(c, "minimize:params-without", lambda e: call(e.minimize, X(), params=ROWS()))
    add(c, "time_solve", lambda e: [call(e.time_solve, X()), call(e.time_solve, X(), 3)])
    add(c, "time_solve:params", lambda e: call(e.time_solve, X(), 2, params=ROWS()), "custom2")

    for c in HAS_SET_PARAMS:
        add(c, "set_params", lambda e: [call(e.set_params, ROWS()), call(e.set_params, [1, 2, 3, 4])], "custom2")
        add(c, "set_params:wrong-size", lambda e: call(e.set_params, np.zeros(3)), "custom2")
        for objective in ("name", "custom0"):
            add(c, f"set_params:without:{objective}", lambda e: call(e.set_params, ROWS()), objective)
    return out


def _statics():
    D, P, G, L, NM, H, S = (N.DEBatchEngine, N.PSOBatchEngine, N.BFGSEngine, N.LMEngine, N.NMEngine,
                            N.NMPSOEngine, N.SANNEngine)
    return [
        ("DEBatchEngine.lds_bytes", lambda: [D.lds_bytes(4, 2), D.lds_bytes(4, 2, 2), D.lds_bytes(4, 2, n_params=0)]),
        ("DEBatchEngine.fits", lambda: [D.fits(4, 2), D.fits(4, 2, 2)]),
        ("PSOBatchEngine.lds_bytes", lambda: [P.lds_bytes(4, 2), P.lds_bytes(4, 2, N.PSO_ACCELERATED, 2)]),
        ("PSOBatchEngine.fits", lambda: [P.fits(4, 2), P.fits(4, 2, N.PSO_ACCELERATED, 2)]),
        ("BFGSEngine.lds_bytes", lambda: [G.lds_bytes(2), G.lds_bytes(2, True), G.lds_bytes(2, False, 2),
                                          G.lds_bytes(2, True, 2, resident=True), G.lds_bytes(2, resident=True)]),
        ("BFGSEngine.has_resident", lambda: G.has_resident()),
        ("BFGSEngine.fits_resident", lambda: [G.fits_resident(2), G.fits_resident(2, True), G.fits_resident(65),
                                              G.fits_resident(2, False, 2), G.fits_resident(2, n_params=4097)]),
        ("BFGSEngine.fits", lambda: [G.fits(2), G.fits(2, True, 2), G.fits(1025), G.fits(2, n_params=4097)]),
        ("LMEngine.lds_bytes", lambda: [L.lds_bytes(2), L.lds_bytes(2, True), L.lds_bytes(2, False, 2)]),
        ("LMEngine.fits", lambda: [L.fits(2), L.fits(2, True, 2), L.fits(1025), L.fits(2, n_params=4097)]),
        ("NMEngine.lds_bytes", lambda: [NM.lds_bytes(2), NM.lds_bytes(2, True), NM.lds_bytes(2, False, 2)]),
        ("NMEngine.fits", lambda: [NM.fits(2), NM.fits(2, True, 2)]),
        ("NMPSOEngine.lds_bytes", lambda: [H.lds_bytes(2), H.lds_bytes(2, 2)]),
        ("NMPSOEngine.fits", lambda: [H.fits(2), H.fits(2, 2)]),
        ("SANNEngine.chains_per_wave", lambda: [S.chains_per_wave(2), S.chains_per_wave(2, 2)]),
        ("SANNEngine.lds_bytes", lambda: [S.lds_bytes(2), S.lds_bytes(2, 2)]),
    ]


def _half_built(make):
    """the engine object of a constructor that raises, closed, dropped and collected"""
    def fn(fake):
        import nlsolver_amd
        cls = getattr(nlsolver_amd, make[0])
        eng = cls.__new__(cls)
        try:
            make[1](eng)
        finally:
            eng.close()
            eng.close()
            handle = getattr(eng, "_h", None)
            del eng
            gc.collect()
        return "no exception", handle and handle.value
    return fn


def _init(cls, objective, **kw):
    """the class's constructor, as make() spells it, run on an instance that exists already"""
    def run(eng):
        args, shape = SHAPE[cls]
        eng.__init__(objective(), *args, **{**shape, **kw})
    return cls, run


# the optional entry points a constructor asks for: symbol -> (class, objective, keywords)
OPTIONAL_AT_CONSTRUCTION = {
    "nlsg_de_ref_create": ("DERefEngine", "name", {}),
    "nlsg_de_ref_create_custom": ("DERefEngine", "custom0", {}),
    "nlsg_de_batch_create": ("DEBatchEngine", "name", {}),
    "nlsg_de_batch_create_custom": ("DEBatchEngine", "custom0", {}),
    "nlsg_de_batch_set_params": ("DEBatchEngine", "custom2", {}),
    "nlsg_pso_batch_create": ("PSOBatchEngine", "name", {}),
    "nlsg_pso_batch_create_custom": ("PSOBatchEngine", "custom0", {}),
    "nlsg_pso_batch_set_params": ("PSOBatchEngine", "custom2", {}),
    "nlsg_nm_create_params": ("NMEngine", "custom2", {}),
    "nlsg_nm_set_params": ("NMEngine", "custom2", {}),
    "nlsg_nmpso_create_params": ("NMPSOEngine", "custom2", {}),
    "nlsg_nmpso_set_params": ("NMPSOEngine", "custom2", {}),
    "nlsg_lm_create_params": ("LMEngine", "custom2", {}),
    "nlsg_lm_set_params": ("LMEngine", "custom2", {}),
    "nlsg_lm_create_link": ("LMEngine", "link", {}),
    "nlsg_lm_create_curve": ("LMEngine", "curve", {}),
    "nlsg_lm_set_curve_data": ("LMEngine", "curve", {}),
    "nlsg_bfgs_create_gradient": ("BFGSEngine", "grad", {}),
    "nlsg_bfgs_create_params": ("BFGSEngine", "custom2", {}),
    "nlsg_bfgs_set_params": ("BFGSEngine", "custom2", {}),
    "nlsg_bfgs_set_params:gradient": ("BFGSEngine", "grad2", {}),
    "nlsg_sann_create_params": ("SANNEngine", "custom2", {}),
    "nlsg_sann_set_params": ("SANNEngine", "custom2", {}),
}
EVERY_OBJECTIVE = dict(OBJECTIVES, quad=quad, tanh=tanh_model, link=link_model, curve=curve_model, grad=CGRAD,
                       grad2=lambda: CGRAD(2))

# every create symbol of a class, with an objective that goes to it
CREATES = {
    "DEEngine": {"nlsg_de_create": "name", "nlsg_de_create_custom": "custom0"},
    "DERefEngine": {"nlsg_de_ref_create": "name", "nlsg_de_ref_create_custom": "custom0"},
    "DEBatchEngine": {"nlsg_de_batch_create": "name", "nlsg_de_batch_create_custom": "custom2"},
    "PSOEngine": {"nlsg_pso_create": "name", "nlsg_pso_create_custom": "custom0"},
    "PSOBatchEngine": {"nlsg_pso_batch_create": "name", "nlsg_pso_batch_create_custom": "custom2"},
    "BFGSEngine": {"nlsg_bfgs_create": "name", "nlsg_bfgs_create:quad": "quad", "nlsg_bfgs_create_custom": "custom0",
                   "nlsg_bfgs_create_params": "custom2", "nlsg_bfgs_create_gradient": "grad"},
    "LMEngine": {"nlsg_lm_create": "name", "nlsg_lm_create:tanh": "tanh", "nlsg_lm_create_custom": "custom0",
                 "nlsg_lm_create_params": "custom2", "nlsg_lm_create_link": "link", "nlsg_lm_create_curve": "curve",
                 "nlsg_lm_set_data": "tanh", "nlsg_lm_set_curve_data": "curve"},
    "NMEngine": {"nlsg_nm_create": "name", "nlsg_nm_create_custom": "custom0", "nlsg_nm_create_params": "custom2"},
    "NMPSOEngine": {"nlsg_nmpso_create": "name", "nlsg_nmpso_create_custom": "custom0",
                    "nlsg_nmpso_create_params": "custom2"},
    "SANNEngine": {"nlsg_sann_create": "name", "nlsg_sann_create_custom": "custom0",
                   "nlsg_sann_create_params": "custom2"},
}


def _model_kw(objective):
    """LMEngine takes batch= and n= with an objective only, BFGSEngine dim= likewise"""
    return objective in ("quad", "tanh", "link", "curve")


def _construct(cls, objective, **kw):
    """construction, what the object then shows, and its release"""
    def fn(fake):
        o = EVERY_OBJECTIVE[objective]()
        if _model_kw(objective):
            eng = getattr(N, cls)(o, *((2,) if cls == "BFGSEngine" else ()), **kw)
        else:
            eng = make(cls, o, **kw)
        shown = {k: getattr(eng, k) for k in ("n_params", "gradient_used", "symmetric", "resident") if hasattr(eng, k)}
        shown["_h"] = eng._h.value
        eng.close()
        shown["closed"] = eng._h.value
        return shown
    return fn


def _lifetime(cls):
    def fn(fake):
        eng = make(cls, "sphere")
        fake.calls.clear()
        eng.close()
        eng.close()
        with make(cls, "sphere") as e:
            inside = e._h.value
        after = e._h.value
        dropped = make(cls, "sphere")
        del dropped
        gc.collect()
        return [inside, after]
    return fn


def _drop_ins():
    x1 = lambda: np.full(2, 0.5)  # noqa: E731
    p1 = [1.0, 2.0]
    out = [
        ("DE.minimize", lambda: call(N.DE("sphere", pop_size=4, max_iter=5).minimize, x1())),
        ("DE.maximize:generator", lambda: call(N.DE("sphere", lambda: 0.5, pop_size=4).maximize, x1())),
        ("DE.minimize:resident", lambda: call(N.DE("sphere", 7, pop_size=4, driver="resident").minimize, x1())),
        ("DE.minimize:reference", lambda: call(N.DE("sphere", N.XorShift(), pop_size=4,
                                                    generation="reference").minimize, x1())),
        ("DE.minimize:params", lambda: call(N.DE(C2(), pop_size=4, params=p1).minimize, x1())),
        ("DE:params-without", lambda: N.DE("sphere", params=p1)),
        ("DE:without-params", lambda: N.DE(C2())),
        ("DE:driver", lambda: N.DE("sphere", driver="fast")),
        ("DE:generation", lambda: N.DE("sphere", generation="fast")),
        ("DE:resident-reference", lambda: N.DE("sphere", N.XorShift(), driver="resident", generation="reference")),
        ("DE:params-reference", lambda: N.DE(C2(), N.XorShift(), generation="reference", params=p1)),
        ("DE:reference-generator", lambda: N.DE("sphere", generation="reference")),
        ("DE.minimize:x", lambda: N.DE("sphere").minimize([0.5, 0.5])),
        ("PSO.minimize", lambda: call(N.PSO("sphere", n_particles=4).minimize, x1())),
        ("PSO.maximize:bounds", lambda: call(N.PSO("sphere", 7, n_particles=4).maximize, x1(), -1.0, 1.0)),
        ("PSO.minimize:resident", lambda: call(N.PSO("sphere", n_particles=4, driver="resident").minimize, x1())),
        ("PSO.minimize:params", lambda: call(N.PSO(C2(), n_particles=4, params=p1).minimize, x1())),
        ("PSO:params-without", lambda: N.PSO("sphere", params=p1)),
        ("PSO:without-params", lambda: N.PSO(C2())),
        ("PSO:driver", lambda: N.PSO("sphere", driver="fast")),
        ("BFGS.minimize", lambda: call(N.BFGS("sphere").minimize, x1())),
        ("BFGS.minimize:batch", lambda: call(N.BFGS("rastrigin", symmetric=True).minimize, X())),
        ("BFGS.minimize:quad", lambda: call(N.BFGS(quad()).minimize, x1())),
        ("BFGS.minimize:resident", lambda: call(N.BFGS(CGRAD(), driver="resident").minimize, X())),
        ("BFGS.minimize:params", lambda: call(N.BFGS(C2(), params=p1).minimize, X())),
        ("BFGS.minimize:params-rows", lambda: call(N.BFGS(C2(), params=ROWS()).minimize, X())),
        ("BFGS.minimize:params-rows-mismatch", lambda: call(N.BFGS(C2(), params=ROWS()).minimize, np.zeros((3, 2)))),
        ("BFGS:params-without", lambda: N.BFGS("sphere", params=p1)),
        ("BFGS:without-params", lambda: N.BFGS(C2())),
        ("BFGS:params-shape", lambda: N.BFGS(C2(), params=[1.0, 2.0, 3.0])),
        ("BFGS:driver", lambda: N.BFGS("sphere", driver="fast")),
        ("BFGS:g", lambda: N.BFGS("sphere", g=lambda x: x)),
        ("BFGS.maximize", lambda: N.BFGS("sphere").maximize(x1())),
        ("LevenbergMarquardt.minimize", lambda: call(N.LevenbergMarquardt("sphere").minimize, x1())),
        ("LevenbergMarquardt.minimize:tanh", lambda: call(N.LevenbergMarquardt(tanh_model()).minimize, X())),
        ("LevenbergMarquardt.minimize:curve", lambda: call(N.LevenbergMarquardt(curve_model()).minimize, np.zeros((2, 3)))),
        ("LevenbergMarquardt.minimize:vector", lambda: call(N.LevenbergMarquardt(CVEC(), solver=1).minimize, X())),
        ("LevenbergMarquardt.minimize:params", lambda: call(N.LevenbergMarquardt(C2(), params=p1).minimize, X())),
        ("LevenbergMarquardt.covariance", lambda: call(N.LevenbergMarquardt(tanh_model()).covariance, X())),
        ("LevenbergMarquardt.stderr", lambda: call(N.LevenbergMarquardt(link_model()).stderr, X(), "absolute")),
        ("LevenbergMarquardt:params-without", lambda: N.LevenbergMarquardt("sphere", params=p1)),
        ("LevenbergMarquardt:without-params", lambda: N.LevenbergMarquardt(C2())),
        ("LevenbergMarquardt:g", lambda: N.LevenbergMarquardt("sphere", g=lambda x: x)),
        ("NelderMead.minimize", lambda: call(N.NelderMead("sphere").minimize, x1())),
        ("NelderMead.maximize:bounds", lambda: call(N.NelderMead("rastrigin").maximize, X(), 1.0, -1.0)),
        ("NelderMead.minimize:params", lambda: call(N.NelderMead(C2(), params=ROWS()).minimize, X())),
        ("NelderMead:params-without", lambda: N.NelderMead("sphere", params=p1)),
        ("NelderMead:without-params", lambda: N.NelderMead(C2())),
        ("NelderMeadPSO.minimize", lambda: call(N.NelderMeadPSO("sphere").minimize, x1())),
        ("NelderMeadPSO.maximize:bounds", lambda: call(N.NelderMeadPSO("sphere", 7).maximize, X(), -1.0, 1.0)),
        ("NelderMeadPSO.minimize:params", lambda: call(N.NelderMeadPSO(C2(), params=p1).minimize, X())),
        ("NelderMeadPSO.minimize:dim1", lambda: call(N.NelderMeadPSO("sphere").minimize, np.zeros(1))),
        ("NelderMeadPSO:params-without", lambda: N.NelderMeadPSO("sphere", params=p1)),
        ("NelderMeadPSO:without-params", lambda: N.NelderMeadPSO(C2())),
        ("SANN.minimize", lambda: call(N.SANN("sphere").minimize, x1())),
        ("SANN.maximize:batch", lambda: call(N.SANN("sphere", 7, max_iter=9).maximize, X())),
        ("SANN.minimize:params", lambda: call(N.SANN(C2(), params=p1).minimize, X())),
        ("SANN:params-without", lambda: N.SANN("sphere", params=p1)),
        ("SANN:without-params", lambda: N.SANN(C2())),
    ]
    return [(i, (lambda f: lambda fake: summary(f()))(f)) for i, f in out]


def _functions():
    """the module-level functions that hand arrays to the library"""
    from nlsolver_amd import de
    Xs, ys = np.full((2, 2, 3), 0.5), np.full((2, 3), 0.25)
    return [
        ("de.jump_table", lambda fake: call(de.jump_table)),
        ("de.pick_donors", lambda fake: call(de.pick_donors, [0.1, 0.2, 0.3, 0.4], 1, 4)),
        ("tinyqr.lm", lambda fake: [call(tinyqr.lm, Xs, ys), call(tinyqr.lm, Xs[0], ys[0], return_ms=True)]),
        ("tinyqr.lm:reference_order", lambda fake: call(tinyqr.lm, Xs, ys, reference_order=True)),
        ("tinyqr.qr_decomposition", lambda fake: call(tinyqr.qr_decomposition, Xs)),
        ("probe_math", lambda fake: call(_capi.probe_math, "log", np.arange(4, dtype=np.uint64))),
    ]


def cases():
    out = []
    for cls in ENGINE_CLASSES:
        for objective in OBJECTIVES:
            out.append(Case(f"{cls}({objective})", _construct(cls, objective)))
        for stream in (None, 0, 0x5A5A):
            out.append(Case(f"{cls}(stream={stream})", _construct(cls, "name", stream=stream)))
            out.append(Case(f"{cls}(custom2, stream={stream})", _construct(cls, "custom2", stream=stream)))
        out.append(Case(f"{cls}:lifetime", _lifetime(cls)))
        for symbol, objective in CREATES[cls].items():
            out.append(Case(f"{cls}:fails:{symbol}", _half_built(_init(cls, EVERY_OBJECTIVE[objective])),
                            fail=[symbol.split(":")[0]]))

    G = "BFGSEngine"
    out.append(Case(f"{G}(quad)", _construct(G, "quad")))
    for objective in ("grad", "grad2"):
        for gradient in N.BFGSEngine.GRADIENTS:
            out.append(Case(f"{G}({objective}, gradient={gradient})", _construct(G, objective, gradient=gradient)))
    for objective in ("name", "quad", "custom0", "custom2"):
        out.append(Case(f"{G}({objective}, gradient=finite_difference)",
                        _construct(G, objective, gradient="finite_difference")))
        out.append(Case(f"{G}({objective}, gradient=analytic)", _construct(G, objective, gradient="analytic")))
    for flag in ("symmetric", "reference_order", "resident"):
        for objective in ("name", "quad", "custom2", "grad"):
            out.append(Case(f"{G}({objective}, {flag})", _construct(G, objective, **{flag: True})))
    out.append(Case(f"{G}(name, every flag)", _construct(G, "name", symmetric=1, reference_order=1, resident=1)))
    out.append(Case(f"{G}(gradient=bogus)", _half_built(_init(G, C0, gradient="bogus"))))
    out.append(Case(f"{G}(name, gradient=analytic):half-built", _half_built(_init(G, lambda: "sphere", gradient="analytic"))))
    out.append(Case(f"{G}(quad, gradient=finite_difference):half-built",
                    _half_built((G, lambda eng: eng.__init__(quad(), 2, gradient="finite_difference")))))
    out.append(Case(f"{G}(custom0, no dim)", _half_built((G, lambda eng: eng.__init__(C0(), 2)))))
    out.append(Case(f"{G}(name, no dim)", _half_built((G, lambda eng: eng.__init__("sphere", 2)))))

    M = "LMEngine"
    for objective in ("tanh", "link", "curve"):
        out.append(Case(f"{M}({objective})", _construct(M, objective)))
        out.append(Case(f"{M}({objective}, stream=0)", _construct(M, objective, stream=0, lam=2.0, up=3.0, down=4.0,
                                                                   max_iter=7, f_delta=1e-9)))
    for solver in (_capi.LM_CHOLESKY, _capi.LM_QR, _capi.LM_CHOLESKY_REFERENCE_ORDER):
        for objective in ("name", "tanh", "custom2"):
            out.append(Case(f"{M}({objective}, solver={solver})", _construct(M, objective, solver=solver)))
    out.append(Case(f"{M}(name, no batch)", _half_built((M, lambda eng: eng.__init__("sphere", n=2)))))
    out.append(Case(f"{M}(custom0, no n)", _half_built((M, lambda eng: eng.__init__(C0(), batch=2)))))

    # keywords that are one engine's own
    out.append(Case("DEEngine(keywords)", _construct(
        "DEEngine", "name", minimize=False, strategy=N.DE_BEST, CR=0.5, F=0.6, eps=1e-5, max_iter=9,
        best_val_no_change=8, seed=77, device=1, shard_lo=1, shard_n=2, trace=True)))
    out.append(Case("DERefEngine(keywords)", _construct(
        "DERefEngine", "name", minimize=False, strategy=N.DE_BEST, CR=0.5, F=0.6, eps=1e-5, max_iter=9,
        best_val_no_change=8, log_capacity=3, device=1)))
    out.append(Case("DEBatchEngine(keywords)", _construct(
        "DEBatchEngine", "name", minimize=False, strategy=N.DE_BEST, CR=0.5, F=0.6, eps=1e-5, max_iter=9,
        best_val_no_change=8, turns_per_launch=4, device=1)))
    out.append(Case("PSOEngine(keywords)", _construct(
        "PSOEngine", "name", type=N.PSO_ACCELERATED, bounded=True, minimize=False, inertia=0.5, cognitive=0.6,
        social=0.7, eps=1e-5, max_iter=9, best_val_no_change=8, seed=77, device=1, shard_lo=1, shard_n=2)))
    out.append(Case("PSOBatchEngine(keywords)", _construct(
        "PSOBatchEngine", "name", type=N.PSO_ACCELERATED, bounded=True, minimize=False, inertia=0.5, cognitive=0.6,
        social=0.7, eps=1e-5, max_iter=9, best_val_no_change=8, turns_per_launch=4, device=1)))
    out.append(Case("BFGSEngine(keywords)", _construct("BFGSEngine", "name", max_iter=9, grad_eps=1e-4, alpha=0.5,
                                                        device=1)))
    out.append(Case("NMEngine(keywords)", _construct(
        "NMEngine", "name", minimize=False, bounded=True, step=0.5, alpha=1.5, gamma=2.5, rho=0.25, sigma=0.75,
        eps=1e-5, max_iter=9, no_change_best_tol=8, restarts=2, device=1, reference_order=True)))
    out.append(Case("NMPSOEngine(keywords)", _construct(
        "NMPSOEngine", "name", minimize=False, bounded=True, alpha=1.5, gamma=2.5, rho=0.25, sigma=0.75,
        inertia=0.5, cognitive=0.6, social=0.7, eps=1e-5, max_iter=9, no_change_best_iter=8, seed=77, inst_lo=3,
        device=1)))
    out.append(Case("SANNEngine(keywords)", _construct(
        "SANNEngine", "name", minimize=False, max_iter=9, temperature_iter=3, temperature_max=2.5, seed=77,
        chain_lo=3, device=1)))

    for id, make, fn in _methods():
        out.append(Case(id, (lambda make, fn: lambda fake: fn(make(fake)))(make, fn)))
    for id, fn in _statics():
        out.append(Case(id, (lambda fn: lambda fake: summary(fn()))(fn)))
    for id, fn in _drop_ins() + _functions():
        out.append(Case(id, fn))

    for symbol, (cls, objective, kw) in OPTIONAL_AT_CONSTRUCTION.items():
        out.append(Case(f"missing:{symbol}", _half_built(_init(cls, EVERY_OBJECTIVE[objective], **kw)),
                        missing=[symbol.split(":")[0]]))
    for symbol in _capi.OPTIONAL_SYMBOLS:
        out.append(Case(f"require:{symbol}", lambda fake, symbol=symbol: _capi.require(symbol) and None,
                        missing=[symbol]))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return out


# ---- the public surface ------------------------------------------------------------------------
def surface():
    """signatures of every exported class's __init__, public methods and static methods, and the public
    names of the engine modules"""
    import importlib
    classes = {}
    for name in sorted(vars(N)):
        cls = getattr(N, name)
        if not inspect.isclass(cls) or name.startswith("_"):
            continue
        sigs = {}
        for attr in ["__init__"] + sorted(a for a in dir(cls) if not a.startswith("_")):
            member = inspect.getattr_static(cls, attr)
            fn = member.__func__ if isinstance(member, (staticmethod, classmethod)) else member
            if inspect.isfunction(fn):
                kind = type(member).__name__ if isinstance(member, (staticmethod, classmethod)) else "method"
                sigs[attr] = f"{kind}{inspect.signature(fn)}"
        classes[name] = sigs
    modules = {m: sorted(a for a in dir(importlib.import_module(f"nlsolver_amd.{m}")) if not a.startswith("_"))
               for m in MODULES}
    return {"classes": classes, "modules": modules, "package": sorted(a for a in dir(N) if not a.startswith("_"))}

"""Shared by tools/record_head_routes.py, test_cpu_head_route_trace.py and test_gpu_head_route_bits.py: the cases that take
``BrainHead`` through every host route (dense, packed, cached, tapped, tapped-and-cached; one head or G = 2; every objective;
with and without target weights, dropout, a penalty per row), the closed-form fit sequences and a buffer-reuse sequence - and
the one runner that drives them, so the recording tool and the tests that replay its files cannot drift apart.

Two things are recorded from the same runner:
* the TRACE (``Recorder``, CPU only): ``head.lib`` is replaced by a proxy that forwards the pure size functions to the real
  library and records every other call instead of making it - entry name, scalars by value, every pointer as
  ``owner+byte_offset`` (owners: a BrainHead attribute or dict entry, a cache tensor, a named runner input, the tensor the
  public call returned; a scratch tensor that lives in a local of a head.py frame has no name that a refactor keeps and is
  recorded as ``local:dtype[numel]``).  NULL is null, the stream is dropped, a pointer without an owner fails the case.
* the BITS (GPU): sha256 of every output the route defines.

Inputs come from CPU generators seeded by the case name; test_cpu_head_route_trace.py holds them to recorded digests."""
import ctypes
import hashlib
import sys
import zlib

import torch

BF = torch.bfloat16
EPS, LAM, DROP_P = 1e-5, 1e-3, 0.25
LOSS_SCALE, L2_SCALE = 0.5, 0.25
SUBJECTS = ("sub-01", "sub-02")
ROUTES = ("dense", "packed", "cached", "tapped1", "tapped3", "tapcached3")
LOSSES = ("mse", "cosine", "pearson")
TAPS = {"tapped1": 1, "tapped3": 3, "tapcached3": 3}
# the one buffer this refactor renames: what the parent calls rows_id is identity_rows
ALIASES = {"rows_id": "identity_rows"}

SHAPE_TRACE = dict(E=256, B=3, S=70, V=40)           # three pooling blocks of 32 rows: partials behind the slabs when dense
SHAPE_1 = dict(E=256, B=3, S=70, V=40)               # MFMA ridge, one loss-partial pair per 16-row tile, skinny dz
SHAPE_2 = dict(E=264, B=17, S=33, V=17)              # scalar ridge, another partial count, B > 16: the wide dz workspace
SHAPE_FIT = dict(E=128, V=17, N=12)                  # 12 clips in two chunks


def _route(name, route, shape, G, loss, tw, keep, l2rows=False):
    return dict(name=name, kind="route", route=route, G=G, loss=loss, tw=tw, keep=keep, l2rows=l2rows, **shape)


def trace_cases():
    """Host-only, so the full product: route x heads x objective x weights x keep_scale, then the options on top of it."""
    out = []
    for r in ROUTES:
        for G in (0, 2):
            for loss in LOSSES:
                for tw in (False, True):
                    for keep in (True, False):
                        out.append(_route(f"{r}/G{G}/{loss}/{'mask' if tw else 'plain'}/{'keep' if keep else 'nokeep'}", r,
                                          SHAPE_TRACE, G, loss, tw, keep))
            out.append(_route(f"{r}/G{G}/mse/l2rows", r, SHAPE_TRACE, G, "mse", False, True, l2rows=True))
    for K in (0, 3):
        for G in (0, 2):
            out.append(dict(name=f"features/K{K}/G{G}", kind="features", K=K, G=G, **SHAPE_TRACE))
    out += fit_cases() + [reuse_case()]
    return out


def bits_cases():
    out = []
    for r in ROUTES:
        for G in (0, 2):
            for loss in LOSSES:
                for tw in (False, True):
                    out.append(_route(f"s1/{r}/G{G}/{loss}/{'mask' if tw else 'plain'}", r, SHAPE_1, G, loss, tw, loss == "mse"))
    for r in ("dense", "cached"):
        for G in (0, 2):
            for loss in ("mse", "pearson"):
                for tw in (False, True):
                    out.append(_route(f"s2/{r}/G{G}/{loss}/{'mask' if tw else 'plain'}", r, SHAPE_2, G, loss, tw, loss == "mse"))
    return out + fit_cases() + [reuse_case()]


def fit_cases():
    return [dict(name=f"fit/{'folds2' if folds else 'nofolds'}/G{G}", kind="fit", folds=folds, G=G, **SHAPE_FIT)
            for folds in (None, 2) for G in (0, 2)]


def reuse_case():
    return dict(name="reuse", kind="reuse", G=0, **SHAPE_TRACE)


# ------------------------------------------------------------------------------------------------------------ inputs
def _gen(case, what):
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(f"{case['name']}/{what}".encode()))


def _bf(t):
    return t.to(BF).float()


def params(case, K=0):
    """bf16-valued fp32 parameters in BrainHead's ``sd`` layout"""
    g, E, V, G = _gen(case, "params"), case["E"], case["V"], case["G"]
    ws, bs = ((G, V, E), (G, V)) if G else ((V, E), (V,))
    sd = {"layer_norm1.weight": 1 + 0.25 * torch.randn(E, generator=g), "layer_norm1.bias": 0.25 * torch.randn(E, generator=g),
          "layer_norm2.weight": 1 + 0.25 * torch.randn(E, generator=g), "layer_norm2.bias": 0.25 * torch.randn(E, generator=g),
          "ridge_layer.linear.weight": torch.randn(*ws, generator=g) / E ** 0.5,
          "ridge_layer.linear.bias": 0.1 * torch.randn(*bs, generator=g)}
    if K > 1:
        sd["layer_mix.weight"] = torch.randn(K, generator=g)
    return {n: _bf(t) for n, t in sd.items()}


def batch(case, B, S, tag="", n_hidden=1, lens=None):
    """hidden (bf16 [B,S,E] each, packed to the live rows with ``lens``), wmask, y, keep, group, tw, l2rows of one batch"""
    g, E, V, H = _gen(case, "batch" + tag), case["E"], case["V"], max(1, case["G"])
    a = {}
    wmask = torch.rand(B, S, generator=g)
    for b in range(B):                                   # a dead leading span per clip, and nothing behind its length
        n = S if lens is None else lens[b]
        wmask[b, :n // 3] = 0
        wmask[b, n:] = 0
    for i in range(n_hidden):
        h = torch.randn(B, S, E, generator=g).to(BF)
        a[f"hidden{i}"] = h.reshape(B * S, E) if lens is None else torch.cat([h[b, :n] for b, n in enumerate(lens)], 0).contiguous()
    a["wmask"] = wmask
    a["y"] = torch.randn(B, V, generator=g)
    a["keep"] = (torch.rand(B, E, generator=g) >= DROP_P).float() / (1 - DROP_P)
    a["group"] = torch.tensor([b % H for b in range(B)], dtype=torch.int32)
    tw = (torch.rand(H, V, generator=g) >= 0.3).float()
    tw[:, :2] = 1                                        # pearson needs two kept targets per head
    a["tw"] = tw
    a["l2rows"] = 1e-3 * (0.5 + torch.rand(H * V, generator=g))
    return a


def cache_arrays(case, N, K=0):
    g, E = _gen(case, "cache"), case["E"]
    return {"cache.pooled": torch.randn(*((K, N, E) if K else (N, E)), generator=g), "cache.sumw": 1 + 10 * torch.rand(N, generator=g)}


def digest(arrays):
    h = hashlib.sha256()
    for k in sorted(arrays):
        t = arrays[k].detach().cpu().contiguous()
        h.update(k.encode())
        h.update(str(t.dtype).encode())
        h.update(t.view(torch.uint8).numpy().tobytes() if t.numel() else b"")
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------------------ the trace
SIZE_FNS = ("_ws_floats", "_ws_doubles", "vlb_head_partial_rows")
_DT = {torch.float32: "f32", torch.float64: "f64", torch.bfloat16: "bf16", torch.int32: "i32", torch.int64: "i64"}


class Recorder:
    """The proxy ``head.lib`` becomes, and the owner table that turns its pointers into names."""

    def __init__(self, real_lib, signatures, pointer_type):
        self.real, self.sig, self.P = real_lib, signatures, pointer_type
        self.names = {}             # the runner's named tensors
        self.head = self.cache = None
        self.calls = []             # of the case so far: (label of the public call) or [entry, args...]
        self._pending = []          # local pointers of the public call in flight: (call, position, address)

    def __getattr__(self, name):
        if name.endswith(SIZE_FNS[:2]) or name == SIZE_FNS[2]:
            return getattr(self.real, name)
        sig = self.sig[name]

        def entry(*args):
            assert len(args) == len(sig), (name, len(args), len(sig))
            call = [name]
            for v, ty in zip(args, sig):
                if ty is not self.P:
                    call.append(v)
                elif v is None:
                    call.append(None)
                elif v == 0:
                    continue                             # the stream
                else:
                    call.append(self._owner(v, call))
            self.calls.append(call)
            if name == "vlb_ridge_cv_select":            # the one result the host indexes with: choice[g] (int32 [V]) <- 0
                ctypes.memset(args[4], 0, 4 * args[8])
            return 0
        return entry

    def _tables(self):
        """(name, tensor) in the order owners are tried: runner inputs, cache, head attributes and their dict entries"""
        out = list(self.names.items())
        if self.cache is not None:
            out += [("cache.pooled", self.cache.pooled), ("cache.sumw", self.cache.sumw)]
        for k in sorted(vars(self.head)):
            v, k = vars(self.head)[k], ALIASES.get(k, k)
            if torch.is_tensor(v):
                out.append((k, v))
            elif isinstance(v, dict):
                for kk in sorted(v, key=str):
                    vs = v[kk] if isinstance(v[kk], (tuple, list)) else [v[kk]]
                    out += [(f"{k}[{kk}]" + (f"[{i}]" if len(vs) > 1 else ""), t) for i, t in enumerate(vs) if torch.is_tensor(t)]
        return out

    @staticmethod
    def _inside(addr, t):
        return t.numel() and t.data_ptr() <= addr < t.data_ptr() + t.numel() * t.element_size()

    @staticmethod
    def _spec(t):
        return f"{_DT[t.dtype]}[{t.numel()}]"

    def _owner(self, addr, call):
        for name, t in self._tables():
            if self._inside(addr, t):
                return f"{name}:{self._spec(t)}+{addr - t.data_ptr()}"
        f = sys._getframe(2)
        while f is not None:                             # a scratch tensor of the method that makes the call
            if f.f_code.co_filename.replace("\\", "/").endswith("phantom_vlb_amd/head.py"):
                for t in _tensors_in(list(f.f_locals.values()), 3):
                    if self._inside(addr, t):
                        self._pending.append((call, len(call), addr))
                        return f"local:{self._spec(t)}+{addr - t.data_ptr()}"
            f = f.f_back
        raise AssertionError(f"{call[0]}: argument {len(call)} points at no known buffer")

    def step(self, label, fn):
        """One public call: its label, the entries it issues; a local that turns out to be what it returned is renamed."""
        self.calls.append(label)
        self._pending = []
        out = fn()
        for call, pos, addr in self._pending:
            for t in _tensors_in([out], 2):
                if self._inside(addr, t):
                    call[pos] = f"returned:{self._spec(t)}+{addr - t.data_ptr()}"
        return out


def _tensors_in(values, depth):
    for v in values:
        if torch.is_tensor(v):
            yield v
        elif depth and isinstance(v, (tuple, list)):
            yield from _tensors_in(v, depth - 1)


class _Plain:
    """the runner without a recorder"""
    names = {}

    def step(self, label, fn):
        return fn()


# ------------------------------------------------------------------------------------------------------------ the runner
def _note(obj, attr, names, key):
    """obj.attr(...) as it is, its (non-None) result remembered as the runner's tensor ``key``"""
    fn = getattr(obj, attr)

    def wrapped(*a, **k):
        out = fn(*a, **k)
        if out is not None:
            names[key] = out
        return out
    setattr(obj, attr, wrapped)


def _make_cache(case, dev, cache_cls, N, K, names):
    cache = cache_cls("train", N, case["E"], dev, layers=K or None)
    cache._alloc()
    arr = cache_arrays(case, N, K)
    cache.pooled.copy_(arr["cache.pooled"])
    cache.sumw.copy_(arr["cache.sumw"])
    cache.valid[:] = True
    _note(cache, "rows", names, "cache_rows")
    return cache, arr


def _make_head(case, dev, head_cls, K, loss, names):
    head = head_cls(case["E"], case["V"], LAM, EPS, dev, sd=params(case, K), loss=loss, readout_layers=list(range(1, K + 1)) if K else None,
                    subjects=list(SUBJECTS) if case["G"] else None)
    _note(head, "_group", names, "group")
    return head


def _grads(head):
    return {f"grads[{n}]": t for n, t in head.grads.items()}


def _route_step(head, cache, route, case, a, dev, rec, out, tag=""):
    """forward + backward of one batch on ``route``; ``out``: the outputs that route defines, as they stand afterwards"""
    B = a["wmask"].shape[0]
    K = TAPS.get(route, 0)
    d = {k: v.to(dev) for k, v in a.items() if torch.is_tensor(v)}
    rec.names.update({k: d[k] for k in d if k.startswith("hidden") or k in ("wmask", "y")})
    keep = d["keep"] if case.get("keep", True) else None
    if keep is not None:
        rec.names["keep"] = keep
    subject = a["group"].tolist() if case["G"] else None
    idx = torch.tensor([(2 * b + 3) % cache.n for b in range(B)]) if cache is not None else None
    lay = a.get("layout")
    if route in ("dense", "packed"):
        if lay is not None:
            rec.names["cu"] = lay.cu
        rec.step(f"forward{tag}", lambda: head.forward(d["hidden0"], d["wmask"], d["y"], keep, layout=lay, subject=subject))
        rec.step("backward(False)", lambda: head.backward(False, LOSS_SCALE, L2_SCALE))
        out["dh"] = rec.step("backward(True)", lambda: head.backward(True, LOSS_SCALE, L2_SCALE))
    elif route == "cached":
        rec.step(f"forward_cached{tag}", lambda: head.forward_cached(cache, idx, d["y"], keep, subject=subject))
        rec.step("backward_cached", lambda: head.backward_cached(LOSS_SCALE, L2_SCALE))
    elif route == "tapcached3":
        rec.step("forward_cached", lambda: head.forward_cached(cache, idx, d["y"], keep, subject=subject))
        rec.step("backward_tapped", lambda: head.backward_tapped(LOSS_SCALE, L2_SCALE))
    else:
        rec.step("begin", lambda: head.begin(*a["wmask"].shape))
        for i in range(K):
            rec.step(f"tap({i})", lambda: head.tap(i, d[f"hidden{i}"], d["wmask"]))
        rec.step("forward_tapped", lambda: head.forward_tapped(d["y"], keep, subject=subject))
        rec.step("backward_tapped", lambda: head.backward_tapped(LOSS_SCALE, L2_SCALE))
        dx = None
        for i in reversed(range(K)):                     # the highest tap writes, the lower ones add
            dx = rec.step(f"dhidden({i})", lambda: head.dhidden(i, d[f"hidden{i}"], into=dx))
            rec.names["dx"] = dx
            out[f"dhidden{i}"] = dx.clone()
    out.update(pred=head.pred, loss_terms=head.loss_terms, pooled_raw=head.pooled_raw, sumw=head.sumw, z=head.z, dz=head.dz,
               dpooled=head.dpooled, **_grads(head))
    if case.get("loss", "mse") != "mse" or head.tw is not None:
        out["loss_aux"] = head.loss_aux
    if K:
        out["alpha"] = head.alpha


def run_case(case, dev, head_cls, cache_cls, rec=None):
    """-> (inputs, outputs): the CPU input tensors by name and the device output tensors by name"""
    rec = rec or _Plain()
    rec.names.clear()
    inputs, out = {}, {}
    kind = case["kind"]
    if kind == "route":
        route = case["route"]
        K, B, S = TAPS.get(route, 0), case["B"], case["S"]
        lens = tuple(max(1, (S * (b + 1)) // B - (b % 2)) for b in range(B))[::-1] if route == "packed" else None
        a = batch(case, B, S, n_hidden=max(1, K), lens=lens)
        head = _make_head(case, dev, head_cls, K, case["loss"], rec.names)
        cache = None
        if route in ("cached", "tapcached3"):
            cache, arr = _make_cache(case, dev, cache_cls, 2 * B + 1, K, rec.names)
            inputs.update(arr)
        rec.head, rec.cache = head, cache
        if lens is not None:
            from phantom_vlb_amd.ops import RowLayout
            a["layout"] = RowLayout(B, S, lens, device=dev)
        if case["tw"]:
            rec.step("set_target_weights", lambda: head.set_target_weights(a["tw"].to(dev)))
        if case["l2rows"]:
            rec.step("set_l2_lambda_rows", lambda: head.set_l2_lambda_rows(a["l2rows"].to(dev)))
        _route_step(head, cache, route, case, a, dev, rec, out)
        inputs.update({k: v for k, v in a.items() if torch.is_tensor(v)}, **params(case, K))
    elif kind == "features":
        K, B = case["K"], case["B"]
        head = _make_head(case, dev, head_cls, K, "mse", rec.names)
        cache, arr = _make_cache(case, dev, cache_cls, 2 * B + 1, K, rec.names)
        rec.head, rec.cache = head, cache
        out["z"] = rec.step("features_cached", lambda: head.features_cached(cache, torch.tensor([4, 0, 5])))
        out.update(pooled_raw=head.pooled_raw, sumw=head.sumw)
        inputs.update(arr, **params(case, K))
    elif kind == "fit":
        N, V, H = case["N"], case["V"], max(1, case["G"])
        head = _make_head(case, dev, head_cls, 0, "mse", rec.names)
        cache, arr = _make_cache(case, dev, cache_cls, N, 0, rec.names)
        rec.head, rec.cache = head, cache
        y = torch.randn(N, V, generator=_gen(case, "y"))
        subject = [(n // 2) % H for n in range(N)]
        rec.step("ridge_stats_begin", lambda: head.ridge_stats_begin(folds=case["folds"], block=2 if case["folds"] else None))
        for c, sl in enumerate((slice(0, 7), slice(7, N))):
            yc = rec.names[f"y{c}"] = y[sl].contiguous().to(dev)
            rec.step(f"ridge_stats_add({c})", lambda: head.ridge_stats_add(cache, torch.arange(N)[sl], yc,
                                                                          subject=subject[sl] if case["G"] else None))
        rec.step("ridge_solve", lambda: head.ridge_solve(0.5))
        solved = {n: head.master[n].clone() for n in ("ridge_layer.linear.weight", "ridge_layer.linear.bias")}
        if case["folds"]:
            cv = rec.step("ridge_cv", lambda: head.ridge_cv([0.25, 4.0], per_target=True))
            rec.names["choice"] = cv["choice"]
            if str(dev) == "cpu":                           # nothing ran: any valid choice serves the trace
                cv["choice"].copy_(torch.arange(H * V, dtype=torch.int32).reshape(H, V) % 2)
            rec.step("ridge_solve_rows", lambda: head.ridge_solve_rows(cv["choice"], cv["grid"]))
            out.update({f"rows/{n}": head.master[n] for n in solved}, choice=cv["choice"])
        out.update({f"solve/{n}": t for n, t in solved.items()})
        inputs.update(arr, y=y, **params(case, 0))
    else:                                                # reuse: one head object, the buffer caps carried from step to step
        head = _make_head(case, dev, head_cls, 0, "mse", rec.names)
        cache, arr = _make_cache(case, dev, cache_cls, 7, 0, rec.names)
        rec.head, rec.cache = head, cache
        inputs.update(arr, **params(case, 0))
        steps = [("dense", 3, 70), ("dense", 2, 33), ("cached", 3, 1), ("cached", 2, 1), ("tw", 0, 0), ("dense", 3, 70)]
        for n, (route, B, S) in enumerate(steps):
            if route == "tw":
                tw = batch(case, 3, 70, tag="0")["tw"]
                rec.step("set_target_weights", lambda: head.set_target_weights(tw.to(dev)))
                continue
            a = batch(case, B, S, tag=str(n))
            inputs.update({f"{n}/{k}": v for k, v in a.items()})
            out = {}
            _route_step(head, cache, route, case, a, dev, rec, out, tag=f"[{n}]")
    return inputs, out


def output_digests(out):
    return {k: digest({k: v}) for k, v in sorted(out.items())}


# ------------------------------------------------------------------------------------------------------------ the two files
def trace_doc(head_mod, cache_cls, patch):
    """Every trace case replayed on the CPU against ``head_mod`` (its ``lib`` and ``_stream`` replaced through
    ``patch(obj, name, value)``) -> the document of tests/golden/head_route_trace.json.  A call is one line,
    ``entry(arg, ...)``; the lines are kept once, in ``calls``, and a case lists their numbers under its public calls."""
    import importlib
    _lib = importlib.import_module("._lib", head_mod.__package__)
    rec = Recorder(head_mod.lib, _lib.SIGNATURES, _lib.P)
    patch(head_mod, "lib", rec)
    patch(head_mod, "_stream", lambda: 0)
    lines, cases = {}, {}
    for case in trace_cases():
        rec.calls = []
        inputs, _ = run_case(case, "cpu", head_mod.BrainHead, cache_cls, rec)
        seq = []
        for c in rec.calls:
            if isinstance(c, str):
                seq.append([c])
            else:
                line = c[0] + "(" + ", ".join("null" if v is None else v if isinstance(v, str) else repr(v) for v in c[1:]) + ")"
                seq[-1].append(lines.setdefault(line, len(lines)))
        cases[case["name"]] = {"inputs": digest(inputs), "steps": [s[0] + ":" + "".join(f" {n}" for n in s[1:]) for s in seq]}
    return {"what": "the C-ABI calls BrainHead issues on every host route (tests/head_route_cases.py), written by "
                    "tools/record_head_routes.py from the head.py that preceded the one host path",
            "calls": list(lines), "cases": cases}


def bits_doc(dev, head_cls, cache_cls):
    """Every bits case run on ``dev`` -> the document of tests/golden/head_route_parent_bits.json"""
    cases = {}
    for case in bits_cases():
        inputs, out = run_case(case, dev, head_cls, cache_cls)
        torch.cuda.synchronize()
        cases[case["name"]] = {"inputs": digest(inputs), "outputs": output_digests(out)}
    return {"what": "sha256 of the inputs and of every output BrainHead defines on every host route "
                    "(tests/head_route_cases.py), written by tools/record_head_routes.py --bits from the head.py that preceded "
                    "the one host path",
            "cases": cases}

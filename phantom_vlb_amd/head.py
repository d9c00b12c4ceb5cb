"""Brain head on libvlb: LN1 -> HRF-weighted pool -> LN2 -> dropout -> ridge linear -> MSE + lambda*||W||^2
(or, opt-in, 1 - mean cosine / Pearson correlation per clip + lambda*||W||^2: ``loss="cosine"`` / ``"pearson"``).

Mirrors the reference's head modules (``layer_norm1``, ``hrf_layer``, ``layer_norm2``, ``dropout``,
``ridge_layer.linear``; src/litmodule/videollama2_vlb_litmodule.py:210-226,245-254 and
src/utils.py:40-73) but runs as the fused vlb_head_fwd / vlb_head_bwd kernels.
Every route is a source of (pooled_raw, sumw), then one tail, then one finisher:
* sources: ``forward`` pools one hidden tensor (fused into vlb_head_fwd for a single head, vlb_head_pool otherwise);
  ``forward_cached`` reads rows of a feature cache; with ``readout_layers`` (§5.3.3) K decoder layers are pooled one by one
  (``begin`` / ``tap``) or gathered from K cache slabs and mixed by softmax(``layer_mix.weight``) (``forward_tapped``);
* ``_tail``: LN2, dropout, the ridge layer and the MSE on that source - vlb_head_fwd_cached, or with ``subjects`` (one ridge
  head per subject on the shared trunk, ``ridge_layer.linear.weight`` [G,V,E], ``subject`` on every forward; §5.3.4)
  vlb_head_fwd_grouped;
* ``_finish``: the objective other than the plain MSE - the correlation objectives of a single head, the weighted one of
  ``set_target_weights`` (§5.3.8) - and the penalty per row of ``set_l2_lambda_rows`` (§5.3.7).
``_backward_tail`` mirrors tail and finisher; ``backward`` adds d loss / d hidden, ``backward_tapped`` the mix's gradient.
Trainable parameters keep an fp32 master (what AdamW updates) and the bf16 copy the kernels read -
the reference stores them in bf16 (``dtype=self.config.dtype``), i.e. the kernels see the same values.
"""
from __future__ import annotations

import math

import torch

from ._lib import check, lib
from .ops import _p, _stream        # _p: an optional tensor as the ABI takes it, NULL for None

BF16 = torch.bfloat16
LOSS_KINDS = {"mse": 0, "cosine": 1, "pearson": 2}      # VLB_LOSS_* of include/vlb.h
HEAD_PARAMS = ("layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias",
               "ridge_layer.linear.weight", "ridge_layer.linear.bias")


def check_loss(loss, num_target):
    """The training objective's name: ``mse`` (the reference's, :302), ``cosine`` (the alternative its training_step
    docstring names, :290-301) or ``pearson`` (cosine of the row-centred prediction and target)."""
    if loss not in LOSS_KINDS:
        raise ValueError(f"loss={loss!r}: expected one of {sorted(LOSS_KINDS)}")
    if loss == "pearson" and num_target < 2:
        raise ValueError(f"loss='pearson' needs num_target >= 2 (got {num_target}): one target has no spread to correlate")


def check_subjects(subjects):
    """``subjects`` as the head, the module and the datamodule take it: None (one head, keyed by the config's ``subject``), or
    a list of two or more distinct subject names -> a tuple."""
    if subjects is None:
        return None
    if isinstance(subjects, (str, bytes)) or not hasattr(subjects, "__iter__"):
        raise ValueError(f"subjects={subjects!r}: a list of subject names is needed (one subject: leave it unset, use `subject`)")
    out = tuple(str(s) for s in subjects)
    if len(out) < 2:
        raise ValueError(f"subjects={list(out)!r}: two or more subjects are needed; a single subject is `subject=...` with "
                         "`subjects` unset")
    if len(set(out)) != len(out):
        raise ValueError(f"subjects={list(out)!r}: a subject is named twice")
    return out


MAX_WEIGHT_LEVELS = 8                # distinct positive weights per head in the weighted closed-form fit: one factorisation each


def target_weight_levels(tw, name=None):
    """The levels of the weighted closed-form fit.  ``tw`` fp32 [H,V] (finite, >= 0) -> {"lvl": [H][V] (the
    rank of a target's weight among its head's distinct positive fp32 values, ascending; -1: masked), "scale": [H][D_h] (fp64,
    Ws / (V w_d) with Ws the exactly rounded sum of the row: what multiplies l2_lambda in that level's solve; 1.0 exactly for a
    constant row), "levels": [H] (D_h)}.  More than ``MAX_WEIGHT_LEVELS`` levels in a head raises with the head named."""
    rows = tw.detach().to("cpu", torch.float32).reshape(-1, tw.shape[-1]).tolist()         # fp32 values, exact as Python floats
    V = len(rows[0])
    out = {"lvl": [], "scale": [], "levels": []}
    for g, row in enumerate(rows):
        vals = sorted({w for w in row if w > 0})
        if len(vals) > MAX_WEIGHT_LEVELS:
            who = name(g) if name is not None else f"head {g}"
            raise ValueError(f"target weights: {who} holds {len(vals)} distinct positive weights; the weighted closed-form fit "
                             f"(ridge_fit_weighted) factors once per distinct weight and takes at most {MAX_WEIGHT_LEVELS}")
        rank = {w: d for d, w in enumerate(vals)}
        ws = math.fsum(row)
        out["lvl"].append([rank[w] if w > 0 else -1 for w in row])
        out["scale"].append([ws / (V * w) for w in vals])
        out["levels"].append(len(vals))
    return out


LAYER_MIX = "layer_mix.weight"       # logits of the learned mix over the tapped layers (K > 1 only), fp32 master [K]
MAX_TAPS = 64                        # MIX_KMAX of head.hip


def check_readout_layers(layers, num_layers: int | None = None):
    """``readout_layers`` as the module takes it: None, or a non-empty list of decoder layers to read the head from.
    k in [1, L] is the output of decoder layer k (HF ``hidden_states[k]``; L = what the head reads by default, after the
    final norm); k in [-L, -1] counts from the end (``-1`` = L).  With ``num_layers`` = L known the list is returned
    normalised and must be strictly ascending; without it only what needs no L is checked and the list comes back as is."""
    if layers is None:
        return None
    if isinstance(layers, (str, bytes)) or not hasattr(layers, "__iter__"):
        raise ValueError(f"readout_layers={layers!r}: a list of decoder layer numbers is needed")
    out = list(layers)
    if not out:
        raise ValueError("readout_layers=[]: at least one decoder layer is needed (None reads the last one, as ever)")
    for k in out:
        if isinstance(k, bool) or not isinstance(k, int):
            raise ValueError(f"readout_layers={out!r}: {k!r} is not an integer layer number")
        if k == 0:
            raise ValueError(f"readout_layers={out!r}: 0 (the spliced embeddings) cannot be tapped; layers count from 1")
    if num_layers is None:
        return out
    L = int(num_layers)
    norm = []
    for k in out:
        if not (1 <= k <= L or -L <= k <= -1):
            raise ValueError(f"readout_layers={out!r}: {k} is outside [1, {L}] and [-{L}, -1] (the decoder has {L} layers)")
        norm.append(k if k > 0 else k + L + 1)
    for prev, k in zip(norm, norm[1:]):
        if k <= prev:
            raise ValueError(f"readout_layers={out!r}: layer {k} after layer {prev} - the (normalised) list {norm} must be "
                             "strictly ascending")
    if len(norm) > MAX_TAPS:
        raise ValueError(f"readout_layers={out!r}: {len(norm)} layers, at most {MAX_TAPS} can be mixed")
    return norm


class BrainHead:
    def __init__(self, dim: int, num_target: int, l2_lambda: float, eps: float, device, sd: dict | None = None,
                 seed: int = 1234, loss: str = "mse", readout_layers=None, subjects=None):
        check_loss(loss, num_target)
        # per-subject ridge heads on the shared trunk; G = 0: one head, the code path as ever
        self.subjects = check_subjects(subjects)
        self.G = 0 if self.subjects is None else len(self.subjects)
        self.loss, self.loss_kind = loss, LOSS_KINDS[loss]
        self.E, self.V, self.l2_lambda, self.eps, self.dev = dim, num_target, float(l2_lambda), float(eps), device
        # taps (normalised by the caller: check_readout_layers with L); K = 0: the fused path on one hidden tensor, as ever
        self.readout_layers = None if readout_layers is None else tuple(int(k) for k in readout_layers)
        self.K = 0 if self.readout_layers is None else len(self.readout_layers)
        if self.readout_layers is not None and not 1 <= self.K <= MAX_TAPS:
            raise ValueError(f"readout_layers={list(self.readout_layers)!r}: 1 to {MAX_TAPS} layers are needed")
        self.param_names = HEAD_PARAMS + ((LAYER_MIX,) if self.K > 1 else ())
        self._tap_cap = None
        self.master: dict[str, torch.Tensor] = {}
        if sd is None:
            gen = torch.Generator(device="cpu").manual_seed(seed)
            bound = 1.0 / math.sqrt(dim)        # nn.Linear default init (kaiming_uniform a=sqrt 5)
            sd = {
                "layer_norm1.weight": torch.ones(dim), "layer_norm1.bias": torch.zeros(dim),
                "layer_norm2.weight": torch.ones(dim), "layer_norm2.bias": torch.zeros(dim),
                "ridge_layer.linear.weight": (torch.rand(num_target, dim, generator=gen) * 2 - 1) * bound,
                "ridge_layer.linear.bias": (torch.rand(num_target, generator=gen) * 2 - 1) * bound,
            }
            if self.G:      # head 0 as a single head of this seed draws it, head g from seed + g; stacked [G,V,E] / [G,V]
                ws_, bs_ = [sd["ridge_layer.linear.weight"]], [sd["ridge_layer.linear.bias"]]
                for g in range(1, self.G):
                    gg = torch.Generator(device="cpu").manual_seed(seed + g)
                    ws_.append((torch.rand(num_target, dim, generator=gg) * 2 - 1) * bound)
                    bs_.append((torch.rand(num_target, generator=gg) * 2 - 1) * bound)
                sd["ridge_layer.linear.weight"], sd["ridge_layer.linear.bias"] = torch.stack(ws_), torch.stack(bs_)
            # the reference creates these modules in bf16 (dtype=self.config.dtype): start from bf16-representable values
            sd = {n: t.to(BF16).float() for n, t in sd.items()}
        for n in self.param_names:
            # handed-in tensors are taken as they are (bf16 checkpoints widen exactly; an fp32 checkpoint of the
            # masters resumes at full precision)
            if n == LAYER_MIX and n not in sd:        # optional on load: a uniform mix, softmax(0)
                self.master[n] = torch.zeros(self.K, dtype=torch.float32, device=device)
                continue
            self.master[n] = sd[n].detach().to(device=device, dtype=torch.float32).contiguous()
        if self.K > 1 and tuple(self.master[LAYER_MIX].shape) != (self.K,):
            raise ValueError(f"{LAYER_MIX}: {tuple(self.master[LAYER_MIX].shape)} handed in, readout_layers="
                             f"{list(self.readout_layers)} needs ({self.K},)")
        want = {"ridge_layer.linear.weight": (self.G, num_target, dim) if self.G else (num_target, dim),
                "ridge_layer.linear.bias": (self.G, num_target) if self.G else (num_target,)}
        for n, shape in want.items():
            if tuple(self.master[n].shape) != shape:
                raise ValueError(f"{n}: {tuple(self.master[n].shape)} handed in, "
                                 f"subjects={None if self.subjects is None else list(self.subjects)!r} needs {shape}")
        self.compute = {n: t.to(BF16) for n, t in self.master.items()}
        self.grads = {n: torch.zeros_like(t) for n, t in self.master.items()}
        self._cap = None
        self.l2_lambda_rows = None        # set_l2_lambda_rows: one penalty per row of the ridge weight
        self.tw = None                    # set_target_weights: fp32 [max(1,G), V] loss weights / masks

    # ------------------------------------------------------------------ per-target loss weights and masks (set_target_weights)
    def set_target_weights(self, tw):
        """``tw`` fp32 on the device, [V] (every head alike) or [H,V] with H = max(1,G) (one row per ridge head): every value
        finite and >= 0, every row with at least one positive value (two for ``pearson``).  The data term becomes the
        weighted one of DESIGN §5.3.8 (a 0/1 row is a mask: the objective on the kept targets alone; targets with weight 0 may
        hold NaN): what ``_finish`` / ``_backward_tail`` then run.  None: back to the unweighted path."""
        if tw is None:
            self.tw = None
            return
        H, V = max(1, self.G), self.V
        if not isinstance(tw, torch.Tensor) or tw.dtype != torch.float32 or tw.device.type != torch.device(self.dev).type or \
                tuple(tw.shape) not in ((V,), (H, V)):
            raise ValueError(f"head: set_target_weights needs an fp32 tensor [{V}] or [{H},{V}] on {self.dev}, got "
                             f"{getattr(tw, 'dtype', type(tw))} {tuple(getattr(tw, 'shape', ()))}")
        tw = tw.detach().reshape(-1, V).expand(H, V).contiguous().clone()
        name = self._head_name
        bad = torch.nonzero(~(torch.isfinite(tw) & (tw >= 0)))
        if bad.numel():
            g, v = (int(i) for i in bad[0])
            raise ValueError(f"head: set_target_weights: {name(g)}, target {v}: weight {float(tw[g, v])} - every weight must be "
                             "finite and >= 0")
        need = 2 if self.loss == "pearson" else 1
        npos = (tw > 0).sum(1).tolist()
        for g, n in enumerate(npos):
            if n < need:
                raise ValueError(f"head: set_target_weights: {name(g)} has {n} target(s) with a positive weight; loss="
                                 f"{self.loss!r} needs at least {need}")
        self.tw = tw
        self._cap = None                  # the next call allocates wstat / dpred with the other buffers

    # ------------------------------------------------------------------ the ABI's pointer blocks, each spelled once
    def _fwd_params(self):
        """the six parameters every forward entry reads: LN1 (w, b), LN2 (w, b), ridge (w, b).  (Literal tuples here and
        below: these run on every call of a latency-bound head.)"""
        c = self.compute
        return (c["layer_norm1.weight"].data_ptr(), c["layer_norm1.bias"].data_ptr(), c["layer_norm2.weight"].data_ptr(),
                c["layer_norm2.bias"].data_ptr(), c["ridge_layer.linear.weight"].data_ptr(),
                c["ridge_layer.linear.bias"].data_ptr())

    def _bwd_params(self):
        """the three parameters every backward entry reads"""
        c = self.compute
        return (c["layer_norm1.weight"].data_ptr(), c["layer_norm2.weight"].data_ptr(),
                c["ridge_layer.linear.weight"].data_ptr())

    def _acts(self):
        """the activations the forward saves and the backward reads"""
        return (self.pooled_raw.data_ptr(), self.sumw.data_ptr(), self.zhat.data_ptr(), self.ln2_rstd.data_ptr(),
                self.z.data_ptr(), self.pred.data_ptr())

    def _grad_ptrs(self):
        """the six parameter gradients: ridge (w, b), LN2 (w, b), LN1 (w, b)"""
        gr = self.grads
        return (gr["ridge_layer.linear.weight"].data_ptr(), gr["ridge_layer.linear.bias"].data_ptr(),
                gr["layer_norm2.weight"].data_ptr(), gr["layer_norm2.bias"].data_ptr(),
                gr["layer_norm1.weight"].data_ptr(), gr["layer_norm1.bias"].data_ptr())

    def _head_name(self, g):
        """how a message names ridge head g"""
        return f"head {g} ({self.subjects[g]!r})" if self.G else "the head"

    # ------------------------------------------------------------------ one l2_lambda per row (set_l2_lambda_rows)
    def set_l2_lambda_rows(self, rows):
        """``rows`` fp32 [R] on the device, R = max(1,G) * V (the rows of ``ridge_layer.linear.weight``), every value finite
        and >= 0: the penalty becomes sum_r rows[r] ||W_r||^2.  Every forward / backward entry is then handed l2_lambda = 0
        and followed by vlb_head_l2_rows_fwd / _bwd on the same stream.  None: back to the scalar ``l2_lambda``."""
        if rows is None:
            self.l2_lambda_rows = None
            return
        if self.loss != "mse":
            raise ValueError(f"head: a penalty per row is defined for the mse objective; this head has loss={self.loss!r}")
        R = max(1, self.G) * self.V
        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float32 or rows.numel() != R or \
                rows.device.type != torch.device(self.dev).type:
            raise ValueError(f"head: set_l2_lambda_rows needs an fp32 tensor of {R} values on {self.dev}, got "
                             f"{getattr(rows, 'dtype', type(rows))} {tuple(getattr(rows, 'shape', ()))}")
        rows = rows.detach().reshape(R).contiguous().clone()
        if not bool((torch.isfinite(rows) & (rows >= 0)).all()):
            raise ValueError("head: set_l2_lambda_rows: every value must be finite and >= 0")
        self.l2_lambda_rows = rows
        self._l2_rows_ws = torch.empty(max(1, lib.vlb_head_l2_rows_ws_doubles(R)), dtype=torch.float64, device=self.dev)

    def _lam(self):
        """the l2_lambda the existing entries are handed: 0 while a penalty per row is in force"""
        return self.l2_lambda if self.l2_lambda_rows is None else 0.0

    def _l2_rows_fwd(self):
        if self.l2_lambda_rows is not None:
            check(lib.vlb_head_l2_rows_fwd(self.compute["ridge_layer.linear.weight"].data_ptr(), self.l2_lambda_rows.data_ptr(),
                                           self._l2_rows_ws.data_ptr(), self.loss_terms.data_ptr(), self.l2_lambda_rows.numel(),
                                           self.E, _stream()), "vlb_head_l2_rows_fwd")

    def _l2_rows_bwd(self, l2_scale):
        if self.l2_lambda_rows is not None:
            check(lib.vlb_head_l2_rows_bwd(self.compute["ridge_layer.linear.weight"].data_ptr(), self.l2_lambda_rows.data_ptr(),
                                           self.grads["ridge_layer.linear.weight"].data_ptr(), self.l2_lambda_rows.numel(), self.E,
                                           float(l2_scale) * 2.0, _stream()), "vlb_head_l2_rows_bwd")

    def _buffers(self, B, S):
        key = (B, S)
        if self._cap != key:
            d, E, V = self.dev, self.E, self.V
            f32 = torch.float32
            self.ws = torch.empty(lib.vlb_head_ws_floats(B, S, E, V), dtype=f32, device=d)
            self.stats = torch.zeros(B, S, 2, dtype=f32, device=d)
            self.pooled_raw = torch.empty(B, E, dtype=f32, device=d)
            self.sumw = torch.empty(B, dtype=f32, device=d)
            self.zhat = torch.empty(B, E, dtype=f32, device=d)
            self.ln2_rstd = torch.empty(B, dtype=f32, device=d)
            self.z = torch.empty(B, E, dtype=BF16, device=d)
            self.pred = torch.empty(B, V, dtype=f32, device=d)
            self.loss_terms = torch.empty(3, dtype=f32, device=d)
            # correlation objectives only: per clip (mu_p, mu_y, sum u^2, sum t^2, sum u t, c_b, 0, 0); (mse, mean c_b)
            self.rowstat = torch.zeros(B, 8, dtype=f32, device=d)
            self.loss_aux = torch.zeros(2, dtype=f32, device=d)
            self.dz = torch.empty(B, E, dtype=f32, device=d)
            self.dpooled = torch.empty(B, E, dtype=f32, device=d)
            self.identity_rows = torch.arange(B, dtype=torch.int32, device=d)      # "cache rows" of a pooled or mixed source
            if self.tw is not None:       # weighted objective only: per clip (.., c_b, W_b, m_b); d loss / d pred
                self.wstat = torch.zeros(B, 8, dtype=f32, device=d)
                self.dpred = torch.empty(B, V, dtype=f32, device=d)
            if self.G:
                self.gws = torch.empty(max(1, lib.vlb_head_grouped_ws_floats(B, E, V, self.G)), dtype=f32, device=d)
                self.pool_src = torch.empty(B, E, dtype=f32, device=d)       # vlb_head_pool's output, the grouped tail's "cache"
                self.pool_sumw = torch.empty(B, dtype=f32, device=d)
            self._cap = key

    # ------------------------------------------------------------------ per-subject heads (subjects=[...])
    def _group(self, subject, B):
        """``subject`` (host ints or a CPU tensor, one head index per clip) checked on the host -> device int32 [B];
        None for a single head.  Nothing is launched before this has passed."""
        if not self.G:
            if subject is not None:
                raise ValueError("head: `subject` given to a head built without `subjects` (one ridge head)")
            return None
        if subject is None:
            raise ValueError(f"head: built with subjects={list(self.subjects)!r}: every call needs `subject`, one index per clip")
        idx = torch.as_tensor(subject).detach().cpu().flatten()
        if idx.numel() != B or idx.is_floating_point() or idx.dtype == torch.bool:
            raise ValueError(f"head: subject has {idx.numel()} entries of {idx.dtype} for a batch of {B}: one integer index per clip")
        idx = idx.to(torch.int64)
        if int(idx.min()) < 0 or int(idx.max()) >= self.G:
            raise ValueError(f"head: subject={idx.tolist()!r} has an index outside [0, {self.G}) (subjects={list(self.subjects)!r})")
        return idx.to(torch.int32).to(self.dev)

    def subject_state_dict(self, name_or_index):
        """One subject's head in the reference's shapes ([V,E], [V], the shared LN tensors; fp32 masters): what a
        per-subject reference module loads."""
        if not self.G:
            raise ValueError("head: subject_state_dict() needs a head built with `subjects`")
        g = name_or_index
        if isinstance(g, str):
            if g not in self.subjects:
                raise ValueError(f"head: subject {g!r} is not one of {list(self.subjects)!r}")
            g = self.subjects.index(g)
        if isinstance(g, bool) or not isinstance(g, int) or not 0 <= g < self.G:
            raise ValueError(f"head: subject index {name_or_index!r} outside [0, {self.G})")
        return {n: (t[g] if n.startswith("ridge_layer.") else t).detach().clone() for n, t in self.master.items()}

    # ------------------------------------------------------------------ sources of (pooled_raw, sumw)
    def _rows_of(self, hidden, wmask, layout):
        """-> (cu, rows) of a hidden tensor under a [B,S] mask: (None, B*S) dense, the layout's own when it is packed"""
        B, S = wmask.shape
        packed = layout is not None and layout.packed
        rows = layout.rows if packed else B * S
        if hidden.numel() != rows * self.E or (packed and (layout.B, layout.S) != (B, S)):
            raise ValueError(f"head: hidden has {hidden.numel() // self.E} rows, layout expects {rows}")
        return (layout.cu if packed else None), rows

    def _pool(self, hidden, wmask, cu, stats, pooled, sumw):
        """LN1 statistics and the pooled vector of one hidden tensor: the pooling half of vlb_head_fwd"""
        B, S = wmask.shape
        check(lib.vlb_head_pool(hidden.data_ptr(), wmask.data_ptr(), self.ws.data_ptr(), stats.data_ptr(), pooled.data_ptr(),
                                sumw.data_ptr(), B, S, self.E, self.eps, _p(cu), _stream()), "vlb_head_pool")

    def _cached_buffers(self, B):
        if self._cap is None or self._cap[0] != B:
            self._buffers(B, 1)           # no pooling workspace needed; buffers of an uncached step of this B serve as they are

    def _gather_taps(self, cache, rows, B):
        """p_stack, tap_sumw <- the K slabs of ``cache`` at ``rows``: the taps' pooled vectors, as ``tap`` leaves them"""
        if cache.layers != self.K:
            raise ValueError(f"head: a feature cache of {cache.layers} slab(s) per clip for {self.K} tapped layer(s)")
        self.begin(B, self._cap[1] if self._cap is not None and self._cap[0] == B else 1)
        for k in range(self.K):
            check(lib.vlb_feature_cache_gather(cache.pooled[k].data_ptr(), cache.sumw.data_ptr(), rows.data_ptr(),
                                               self.p_stack[k].data_ptr(), self.tap_sumw.data_ptr(), B, self.E, cache.n,
                                               _stream()), "vlb_feature_cache_gather")

    def _mix(self, B):
        """alpha = softmax(layer_mix.weight), mixed = sum_k alpha_k P_k"""
        check(lib.vlb_head_mix_fwd(self.p_stack.data_ptr(), self.compute[LAYER_MIX].data_ptr() if self.K > 1 else None,
                                   self.alpha.data_ptr(), self.mixed.data_ptr(), self.K, B, self.E, _stream()),
              "vlb_head_mix_fwd")

    # ------------------------------------------------------------------ one tail, one finisher, one backward tail
    def _tail(self, src_pooled, src_sumw, rows, n_rows, y, keep_scale, group):
        """(src rows -> pooled_raw, sumw), LN2, dropout, the ridge layer of one head (``group`` None) or of every clip's own
        (DESIGN §5.3.4), the objective -> (pred f32 [B,V], loss_terms f32[3])"""
        B = y.shape[0]
        self._saved_tail = (y, keep_scale, group)
        if group is None:
            check(lib.vlb_head_fwd_cached(src_pooled.data_ptr(), src_sumw.data_ptr(), rows.data_ptr(), *self._fwd_params(),
                                          y.data_ptr(), _p(keep_scale), self.ws.data_ptr(), *self._acts(),
                                          self.loss_terms.data_ptr(), B, self.E, self.V, n_rows, self.eps, self._lam(),
                                          _stream()), "vlb_head_fwd_cached")
        else:       # the entry finishes a correlation objective itself; the weighted one starts from its MSE partials
            check(lib.vlb_head_fwd_grouped(src_pooled.data_ptr(), src_sumw.data_ptr(), rows.data_ptr(), *self._fwd_params(),
                                           y.data_ptr(), _p(keep_scale), group.data_ptr(), self.gws.data_ptr(), *self._acts(),
                                           self.rowstat.data_ptr(), self.loss_terms.data_ptr(), self.loss_aux.data_ptr(), B,
                                           self.E, self.V, self.G, n_rows, self.eps, self._lam(),
                                           self.loss_kind if self.tw is None else LOSS_KINDS["mse"], _stream()),
                  "vlb_head_fwd_grouped")
        return self._finish(y, B, 0, group)

    def _finish(self, y, B, S, group):
        """The objective, on the pred and ridge partials the forward just left (S: where they sit in the workspace - behind
        the pooling slabs of vlb_head_fwd, 0 after the tail; group: the grouped tail's, its workspace is gws), then the
        penalty per row -> (pred, loss_terms)."""
        if self.tw is not None:           # loss_terms, loss_aux, wstat <- the weighted objective
            ws = self.ws if group is None else self.gws
            check(lib.vlb_head_wloss_fwd(self.pred.data_ptr(), y.data_ptr(), self.tw.data_ptr(), _p(group), ws.data_ptr(),
                                         self.wstat.data_ptr(), self.loss_terms.data_ptr(), self.loss_aux.data_ptr(), B, S,
                                         self.E, self.V, max(1, self.G), self.loss_kind, self._lam(), _stream()),
                  "vlb_head_wloss_fwd")
        elif self.loss_kind and group is None:
            self._loss_fwd(y, B, S)
        self._l2_rows_fwd()
        return self.pred, self.loss_terms

    def _loss_fwd(self, y, B, S):
        """loss_terms[0], [2] <- the chosen correlation objective of a single head"""
        check(lib.vlb_head_loss_fwd(self.pred.data_ptr(), y.data_ptr(), self.ws.data_ptr(), self.rowstat.data_ptr(),
                                    self.loss_terms.data_ptr(), self.loss_aux.data_ptr(), B, S, self.E, self.V,
                                    self.loss_kind, self._lam(), _stream()), "vlb_head_loss_fwd")

    def _backward_tail(self, loss_scale, l2_scale):
        """Parameter gradients (self.grads, overwritten) and dpooled = d loss / d pooled_raw of the last tail or forward."""
        y, keep_scale, group = self._saved_tail
        B = y.shape[0]
        if self.tw is not None:
            ws = self.ws if group is None else self.gws
            check(lib.vlb_head_bwd_wloss(*self._bwd_params(), y.data_ptr(), self.tw.data_ptr(), _p(keep_scale), _p(group),
                                         *self._acts(), self.wstat.data_ptr(), self.dpred.data_ptr(), *self._grad_ptrs(),
                                         ws.data_ptr(), self.dz.data_ptr(), self.dpooled.data_ptr(), B, self.E, self.V,
                                         max(1, self.G), self._lam(), float(loss_scale), float(l2_scale), self.loss_kind,
                                         _stream()), "vlb_head_bwd_wloss")
        elif group is not None:
            check(lib.vlb_head_bwd_grouped(*self._bwd_params(), y.data_ptr(), _p(keep_scale), group.data_ptr(), *self._acts(),
                                           *self._grad_ptrs(), self.gws.data_ptr(), self.dz.data_ptr(), self.dpooled.data_ptr(),
                                           self.rowstat.data_ptr(), B, self.E, self.V, self.G, self.eps, self._lam(),
                                           float(loss_scale), float(l2_scale), self.loss_kind, _stream()), "vlb_head_bwd_grouped")
        else:
            fn, tail, what = lib.vlb_head_bwd_cached, (), "vlb_head_bwd_cached"
            if self.loss_kind:
                fn, tail, what = lib.vlb_head_bwd_cached_loss, (self.loss_kind, self.rowstat.data_ptr()), "vlb_head_bwd_cached_loss"
            check(fn(*self._bwd_params(), y.data_ptr(), _p(keep_scale), *self._acts(), *self._grad_ptrs(), self.ws.data_ptr(),
                     self.dz.data_ptr(), self.dpooled.data_ptr(), B, self.E, self.V, self.eps, self._lam(), float(loss_scale),
                     float(l2_scale), _stream(), *tail), what)
        self._l2_rows_bwd(l2_scale)

    def _dhidden(self, hidden, wmask, stats, dpooled, dx, cu, rows, add):
        """dx (bf16 [rows,E]) <- or += one hidden tensor's term of d loss / d hidden: vlb_head_bwd's last launch"""
        B, S = wmask.shape
        check(lib.vlb_head_dhidden(hidden.data_ptr(), wmask.data_ptr(), stats.data_ptr(), dpooled.data_ptr(), dx.data_ptr(), B, S,
                                   self.E, _p(cu), rows, add, _stream()), "vlb_head_dhidden")

    # ------------------------------------------------------------------ one hidden tensor
    def forward(self, hidden, wmask, y, keep_scale=None, layout=None, subject=None):
        """hidden bf16 [B*S,E] (or [B,S,E]; packed rows with a packed ``layout``), wmask f32 [B,S] (always
        dense), y f32 [B,V] -> (pred f32 [B,V], loss_terms f32[3]).  ``subject``: the head index of every clip, for a head
        built with ``subjects`` (then: vlb_head_pool, the tail on identity rows; backward adds vlb_head_dhidden)."""
        B, S = wmask.shape
        group = self._group(subject, B)
        cu, rows = self._rows_of(hidden, wmask, layout)
        self._buffers(B, S)
        self._saved = (hidden, wmask, y, keep_scale, cu, rows)
        if group is not None:
            self._pool(hidden, wmask, cu, self.stats, self.pool_src, self.pool_sumw)
            return self._tail(self.pool_src, self.pool_sumw, self.identity_rows, B, y, keep_scale, group)
        self._saved_tail = (y, keep_scale, None)
        check(lib.vlb_head_fwd(hidden.data_ptr(), wmask.data_ptr(), *self._fwd_params(), y.data_ptr(), _p(keep_scale),
                               self.ws.data_ptr(), self.stats.data_ptr(), *self._acts(), self.loss_terms.data_ptr(), B, S,
                               self.E, self.V, self.eps, self._lam(), _p(cu), _stream()), "vlb_head_fwd")
        return self._finish(y, B, S, None)

    def backward(self, need_dhidden: bool, loss_scale: float = 1.0, l2_scale: float = 1.0):
        """Fills self.grads (fp32, overwritten) and returns d loss / d hidden (bf16) or None."""
        hidden, wmask, y, keep_scale, cu, rows = self._saved
        B, S = wmask.shape
        dh = torch.empty(rows, self.E, dtype=BF16, device=self.dev) if need_dhidden else None
        if self.G or self.tw is not None:
            self._backward_tail(loss_scale, l2_scale)
            if need_dhidden:
                self._dhidden(hidden, wmask, self.stats, self.dpooled, dh, cu, rows, 0)
            return dh
        # one head, no weights: the fused entry (it refuses a wrong row count before its first launch)
        fn, tail, what = lib.vlb_head_bwd, (), "vlb_head_bwd"
        if self.loss_kind:
            fn, tail, what = lib.vlb_head_bwd_loss, (self.loss_kind, self.rowstat.data_ptr()), "vlb_head_bwd_loss"
        check(fn(hidden.data_ptr(), wmask.data_ptr(), *self._bwd_params(), y.data_ptr(), _p(keep_scale),
                 self.stats.data_ptr(), *self._acts(), *self._grad_ptrs(), self.ws.data_ptr(), self.dz.data_ptr(),
                 self.dpooled.data_ptr(), _p(dh), B, S, self.E, self.V, self.eps, self._lam(), float(loss_scale),
                 float(l2_scale), _p(cu), rows, _stream(), *tail), what)
        self._l2_rows_bwd(l2_scale)
        return dh

    # ------------------------------------------------------------------ frozen-backbone feature cache (feature_cache.py)
    def forward_cached(self, cache, indices, y, keep_scale=None, subject=None):
        """The head forward of a batch whose (pooled_raw, sumw) sit in ``cache`` rows ``indices`` (host int64 [B]):
        -> (pred f32 [B,V], loss_terms f32[3]), the same bits vlb_head_fwd gives for the same (pooled_raw, sumw)."""
        B = y.shape[0]
        group = self._group(subject, B)
        rows = cache.rows(indices)
        if rows.numel() != B:
            raise ValueError(f"head: {rows.numel()} cache rows for a batch of {B}")
        if self.K:                        # K slabs per clip -> the taps' pooled vectors, then the tapped forward as uncached
            self._gather_taps(cache, rows, B)
            return self.forward_tapped(y, keep_scale, subject)
        self._cached_buffers(B)
        return self._tail(cache.pooled, cache.sumw, rows, cache.n, y, keep_scale, group)

    def backward_cached(self, loss_scale: float = 1.0, l2_scale: float = 1.0):
        """Parameter gradients after forward_cached (fills self.grads, overwritten; no gradient wrt hidden)."""
        self._backward_tail(loss_scale, l2_scale)

    # ------------------------------------------------------------------ readout from chosen decoder layers (readout_layers)
    # Per step: begin(B, S); tap(i, hidden_i, wmask, layout) as each tapped layer's output exists (only its LN1 statistics
    # [B,S,2] and pooled vector P_i [B,E] are kept, never the tensor); forward_tapped(y, keep); backward_tapped(...);
    # dhidden(i, hidden_i, into) for the taps' terms of d loss / d hidden, highest tap first (write), lower ones added.
    def begin(self, B, S):
        if not self.K:
            raise RuntimeError("head: begin() / tap() are the readout_layers API; this head reads one hidden tensor (forward())")
        if self._cap is None or self._cap[0] != B or self._cap[1] < S:
            self._buffers(B, S)
        if self._tap_cap != (B, S):
            d, E, K, f32 = self.dev, self.E, self.K, torch.float32
            self.tap_stats = torch.zeros(K, B, S, 2, dtype=f32, device=d)
            self.p_stack = torch.empty(K, B, E, dtype=f32, device=d)           # P_k: pooled_raw of tap k
            self.tap_sumw = torch.empty(B, dtype=f32, device=d)                # the same for every tap (same mask, same order)
            self.mixed = torch.empty(B, E, dtype=f32, device=d)                # sum_k alpha_k P_k
            self.alpha = torch.empty(K, dtype=f32, device=d)
            self.draw_stack = torch.empty(K, B, E, dtype=f32, device=d)        # alpha_k * d loss / d pooled_raw
            self.mix_ws = torch.empty(max(1, lib.vlb_head_mix_ws_floats(K, B, E)), dtype=f32, device=d)
            self._d_a1 = torch.empty(1, dtype=f32, device=d)                   # K = 1: no logit, its (zero) gradient lands here
            self._tap_cap = (B, S)
        self._tap_meta = None

    def tap(self, i, hidden, wmask, layout=None):
        """LN1 statistics and pooled vector of tap i (0-based position in ``readout_layers``) from its hidden tensor
        (bf16 rows x E, dense [B*S] or packed by ``layout``): the pooling half of vlb_head_fwd."""
        B, S = wmask.shape
        cu, rows = self._rows_of(hidden, wmask, layout)
        if self._tap_cap != (B, S) or not 0 <= i < self.K:
            raise ValueError(f"head: tap({i}) of a [{B},{S}] mask after begin{self._tap_cap} with {self.K} tap(s)")
        self._tap_meta = (wmask, cu, rows)
        self._pool(hidden, wmask, cu, self.tap_stats[i], self.p_stack[i], self.tap_sumw)

    def forward_tapped(self, y, keep_scale=None, subject=None):
        """alpha = softmax(layer_mix.weight), pooled_raw = sum_k alpha_k P_k, then the tail of the head on
        (pooled_raw, sumw) -> (pred f32 [B,V], loss_terms f32[3])."""
        B = y.shape[0]
        group = self._group(subject, B)
        self._mix(B)
        return self._tail(self.mixed, self.tap_sumw, self.identity_rows, B, y, keep_scale, group)

    def backward_tapped(self, loss_scale: float = 1.0, l2_scale: float = 1.0):
        """Head gradients on the mixed pooled vector (fills self.grads), then the mix's own:
        grads['layer_mix.weight'] (K > 1; written) and draw_stack[k] = alpha_k * d loss / d pooled_raw for dhidden()."""
        self._backward_tail(loss_scale, l2_scale)
        B = self._saved_tail[0].shape[0]
        d_a = self.grads[LAYER_MIX] if self.K > 1 else self._d_a1
        check(lib.vlb_head_mix_bwd(self.p_stack.data_ptr(), self.dpooled.data_ptr(), self.alpha.data_ptr(), d_a.data_ptr(),
                                   self.draw_stack.data_ptr(), self.mix_ws.data_ptr(), self.K, B, self.E, _stream()),
              "vlb_head_mix_bwd")

    def dhidden(self, i, hidden, into=None):
        """Tap i's term of d loss / d hidden_i (bf16 [rows,E]) from its hidden tensor, statistics and draw_stack[i].
        ``into`` None: a fresh tensor, zero-weight rows zeroed (vlb_head_bwd's last launch).  ``into`` = dx: added to dx
        in place on the rows with a non-zero weight; the others are not touched."""
        wmask, cu, rows = self._tap_meta
        if hidden.numel() != rows * self.E or (into is not None and (into.numel() != rows * self.E or into.dtype != BF16)):
            raise ValueError(f"head: dhidden({i}) needs bf16 [{rows},{self.E}] tensors")
        dx = torch.empty(rows, self.E, dtype=BF16, device=self.dev) if into is None else into
        self._dhidden(hidden, wmask, self.tap_stats[i], self.draw_stack[i], dx, cu, rows, 0 if into is None else 1)
        return dx

    # ------------------------------------------------------------------ closed-form ridge fit (ridge_fit="closed_form")
    # With loss="mse", the LN parameters (and the mix) held fixed and dropout off, the objective over N clips is a ridge
    # regression in (ridge_layer.linear.weight, .bias); DESIGN §5.3.5.  ridge_stats_begin(); ridge_stats_add(...) per chunk of
    # cached clips; ridge_solve() -> the minimiser, written into the fp32 masters and their bf16 copies.  All fp64 on the device.
    def ridge_stats_begin(self, folds=None, block=None, weighted=False):
        """Allocate and zero the fp64 sums (G [E,E], C [V,E], sz [E], sy [V]), one set per head.  ``folds=K`` (with
        ``block``): one set per (head, fold) plus syy [V] = sum y^2, for ``ridge_cv``; a head's m-th clip
        (its rank among the clips that head has received so far) goes to fold ``(m // block) % K``.
        ``weighted=True`` takes ``self.tw`` as it is at this call: the sums skip the masked targets (which may
        hold NaN) and ``ridge_solve`` / ``ridge_cv`` / ``ridge_solve_rows`` minimise the weighted objective of §5.3.8, one
        factorisation per distinct positive weight of a head (at most ``MAX_WEIGHT_LEVELS``).  Without weights set it changes
        nothing."""
        if self.loss != "mse":
            raise ValueError(f"head: the closed-form ridge fit minimises the mse objective; this head has loss={self.loss!r}")
        if self.tw is not None and not weighted:
            raise ValueError("head: the closed-form ridge fit does not take target weights (a mask would need NaN-tolerant Gram "
                             "columns, general weights one factorisation per distinct weight) unless it is begun with "
                             "weighted=True (ridge_fit_weighted): set_target_weights(None) first, or opt in")
        H, E, V, d, f64 = max(1, self.G), self.E, self.V, self.dev, torch.float64
        wst = {}
        if self.tw is not None:
            lv = target_weight_levels(self.tw, self._head_name)
            keep = self.tw > 0
            wst = {"tw": self.tw.clone(), "lvl": torch.tensor(lv["lvl"], dtype=torch.int32, device=d), "scale": lv["scale"],
                   "keep": keep, "kept": [int(n) for n in keep.sum(1).tolist()],
                   "kept_idx": [torch.nonzero(keep[g]).flatten() for g in range(H)]}
        if folds is not None:
            K, blk = int(folds), 1 if block is None else int(block)
            if K < 2 or blk < 1:
                raise ValueError(f"head: ridge_stats_begin: folds={folds}, block={block}: folds >= 2 and block >= 1 are needed")
            self._ridge = {"G": torch.zeros(H, K, E, E, dtype=f64, device=d), "C": torch.zeros(H, K, V, E, dtype=f64, device=d),
                           "sz": torch.zeros(H, K, E, dtype=f64, device=d), "sy": torch.zeros(H, K, V, dtype=f64, device=d),
                           "syy": torch.zeros(H, K, V, dtype=f64, device=d), "n": [0] * H, "n_fold": [[0] * K for _ in range(H)],
                           "folds": K, "block": blk, **wst}
            return
        self._ridge = {"G": torch.zeros(H, E, E, dtype=f64, device=d), "C": torch.zeros(H, V, E, dtype=f64, device=d),
                       "sz": torch.zeros(H, E, dtype=f64, device=d), "sy": torch.zeros(H, V, dtype=f64, device=d), "n": [0] * H,
                       **wst}

    def ridge_stats_end(self):
        """Free the sums (and the last solve's workspaces)."""
        self._ridge = None

    def features_cached(self, cache, indices):
        """z bf16 [n,E] of the cached clips ``indices``: what the ridge layer reads in ``forward_cached`` with
        ``keep_scale=None`` (same gather, same mix, same LN2 launch: the same bits), and nothing after it.  The tensor is the
        head's own ``z`` buffer: the next call overwrites it."""
        rows = cache.rows(indices)
        B = rows.numel()
        if self.K:
            self._gather_taps(cache, rows, B)
            self._mix(B)
            src, sw, rows, n_rows = self.mixed, self.tap_sumw, self.identity_rows, B
        else:
            if cache.layers is not None:
                raise ValueError(f"head: a feature cache of {cache.layers} slab(s) per clip for a head without readout_layers")
            self._cached_buffers(B)
            src, sw, n_rows = cache.pooled, cache.sumw, cache.n
        check(lib.vlb_head_features_cached(src.data_ptr(), sw.data_ptr(), rows.data_ptr(), *self._fwd_params()[:4],
                                           *self._acts()[:5], B, self.E, n_rows, self.eps, _stream()),
              "vlb_head_features_cached")
        return self.z

    def ridge_stats_add(self, cache, indices, y, subject=None):
        """Add a chunk of cached clips (``indices``: host int64 [n]; ``y`` fp32 [n,V] on the device; ``subject``: one head
        index per clip for a head built with ``subjects``) to the sums.  Checked on the host like ``forward_cached``; with
        ``subjects`` the chunk is partitioned on the host and each part goes to its own head's sums, in index order."""
        st = getattr(self, "_ridge", None)
        if st is None:
            raise RuntimeError("head: ridge_stats_add() before ridge_stats_begin()")
        idx = torch.as_tensor(indices).detach().cpu().flatten().to(torch.int64)
        n = idx.numel()
        if y.dim() != 2 or tuple(y.shape) != (n, self.V) or y.dtype != torch.float32 or y.device.type != torch.device(self.dev).type:
            raise ValueError(f"head: ridge_stats_add needs y fp32 [{n},{self.V}] on {self.dev}, got {y.dtype} {tuple(y.shape)} on {y.device}")
        group = self._group(subject, n)
        if group is None:
            parts = [(0, idx, y.contiguous())]
        else:
            g_host = torch.as_tensor(subject).detach().cpu().flatten().to(torch.int64)
            parts = []
            for g in range(self.G):
                sel = torch.nonzero(g_host == g).flatten()
                if sel.numel():
                    parts.append((g, idx[sel], y.index_select(0, sel.to(y.device)).contiguous()))
        if "folds" in st:
            return self._ridge_stats_add_folds(st, cache, parts)
        for g, ids, yy in parts:
            self._ridge_accumulate(st, g, cache, ids, yy)
            st["n"][g] += ids.numel()

    def _ridge_accumulate(self, st, at, cache, ids, y):
        """the sums at ``at`` (a head, or a (head, fold)) += the cached clips ``ids`` with targets ``y``"""
        z = self.features_cached(cache, ids)
        if "tw" in st:          # weighted stats (§5.3.9): y through a select on the head's own weight row
            g = at[0] if isinstance(at, tuple) else at
            check(lib.vlb_ridge_gram_accumulate_masked(z.data_ptr(), y.data_ptr(), self.V, st["tw"][g].data_ptr(),
                                                       st["G"][at].data_ptr(), st["C"][at].data_ptr(), st["sz"][at].data_ptr(),
                                                       st["sy"][at].data_ptr(), ids.numel(), self.E, self.V, _stream()),
                  "vlb_ridge_gram_accumulate_masked")
            return
        check(lib.vlb_ridge_gram_accumulate(z.data_ptr(), y.data_ptr(), self.V, st["G"][at].data_ptr(), st["C"][at].data_ptr(),
                                            st["sz"][at].data_ptr(), st["sy"][at].data_ptr(), ids.numel(), self.E, self.V,
                                            _stream()), "vlb_ridge_gram_accumulate")

    def _head_totals(self, st, g):
        """(G, C, sz, sy) of head g; with folds its folds' sums added in ascending order (skip = -1)"""
        return self._ridge_fold_sums(st, g, -1) if "folds" in st else (st["G"][g], st["C"][g], st["sz"][g], st["sy"][g])

    @staticmethod
    def _ridge_grid(what, grid):
        grid = [float(x) for x in grid]
        if not grid or not all(math.isfinite(x) and x > 0 for x in grid):
            raise ValueError(f"head: {what}: grid={grid!r}: one or more positive values are needed")
        return grid

    def _write_ridge(self, W, b):
        """the fitted (W, b) into the fp32 masters and their bf16 copies"""
        wn, bn = "ridge_layer.linear.weight", "ridge_layer.linear.bias"
        self.master[wn].copy_(W.view(self.master[wn].shape))
        self.master[bn].copy_(b.view(self.master[bn].shape))
        self.compute[wn].copy_(self.master[wn])         # fp32 -> bf16, round to nearest even: what AdamW's rewrite gives too
        self.compute[bn].copy_(self.master[bn])

    def ridge_solve(self, l2_lambda=None):
        """Minimise the mse objective over the accumulated clips in (weight, bias), per head: one fp64 Cholesky factorisation
        and solve each.  -> a list (one entry per head) of {"subject", "n", "info", "l2_lambda"}.  Everything is solved
        first; a head without clips, a singular system (``l2_lambda`` 0 with n <= E) or a failed pivot (``info`` != 0) raises
        with the head and the pivot named and leaves every parameter as it was.  Otherwise the fp32 masters and their bf16
        copies are written.  The sums are only read: another ``l2_lambda`` solves again from them.  With folds active the
        head's sums are its folds' added in ascending order.  With weighted stats the weighted objective is
        minimised: per head and level one vlb_ridge_solve_rows with ``l2_lambda * scale`` writes that level's rows, masked rows
        are exactly 0, and the dicts gain "kept" (targets with a positive weight) and "levels"."""
        st = getattr(self, "_ridge", None)
        if st is None:
            raise RuntimeError("head: ridge_solve() before ridge_stats_begin()")
        lam = self.l2_lambda if l2_lambda is None else float(l2_lambda)
        H, E, V, d = max(1, self.G), self.E, self.V, self.dev
        name = self._head_name
        if lam < 0:
            raise ValueError(f"head: ridge_solve: l2_lambda = {lam} is negative")
        for g in range(H):
            if st["n"][g] == 0:
                raise ValueError(f"head: ridge_solve: {name(g)} has no clips (N = 0): nothing to fit it to")
            if not lam > 0 and st["n"][g] <= E:
                raise ValueError(f"head: ridge_solve: {name(g)} has N = {st['n'][g]} <= E = {E} clips and l2_lambda = {lam}: the "
                                 "centred Gram matrix is singular; set l2_lambda > 0")
        A = torch.empty(E, E, dtype=torch.float64, device=d)
        X = torch.empty(H, V, E, dtype=torch.float64, device=d)
        wt = "tw" in st         # weighted stats (§5.3.9): one row-select solve per (head, level) into zeroed scratch
        jobs = [(g, lv) for g in range(H) for lv in range(len(st["scale"][g]))] if wt else [(g, None) for g in range(H)]
        W = (torch.zeros if wt else torch.empty)(H, V, E, dtype=torch.float32, device=d)
        b = (torch.zeros if wt else torch.empty)(H, V, dtype=torch.float32, device=d)
        info = torch.zeros(len(jobs), dtype=torch.int32, device=d)
        for j, (g, lv) in enumerate(jobs):
            Gs, Cs, szs, sys_ = self._head_totals(st, g)
            if lv is None:
                check(lib.vlb_ridge_solve(Gs.data_ptr(), Cs.data_ptr(), szs.data_ptr(), sys_.data_ptr(),
                                          st["n"][g], lam, A.data_ptr(), X[g].data_ptr(), W[g].data_ptr(), b[g].data_ptr(),
                                          info[g:].data_ptr(), E, V, _stream()), "vlb_ridge_solve")
            else:
                check(lib.vlb_ridge_solve_rows(Gs.data_ptr(), Cs.data_ptr(), szs.data_ptr(), sys_.data_ptr(), st["n"][g],
                                               lam * st["scale"][g][lv], A.data_ptr(), X[g].data_ptr(), W[g].data_ptr(),
                                               b[g].data_ptr(), info[j:].data_ptr(), E, V, st["lvl"][g].data_ptr(), lv, _stream()),
                      "vlb_ridge_solve_rows")
        by_job = info.tolist()                          # the one device read of the solve
        infos = [next((v for (gg, _), v in zip(jobs, by_job) if gg == g and v), 0) for g in range(H)]
        st["X"] = X                                     # the fp64 solutions, for inspection (weighted: the last level's)
        for g in range(H):
            if infos[g] < 0:
                raise ValueError(f"head: ridge_solve: {name(g)}: target column {-infos[g] - 1} holds a NaN or Inf (info = "
                                 f"{infos[g]}, N = {st['n'][g]}); the parameters are unchanged")
            if infos[g]:
                raise ValueError(f"head: ridge_solve: {name(g)}: pivot {infos[g]} of {E} is not positive (info = {infos[g]}, "
                                 f"N = {st['n'][g]}, l2_lambda = {lam}): a larger l2_lambda, or NaN in the targets")
        self._write_ridge(W, b)
        out = [{"subject": self.subjects[g] if self.G else None, "n": st["n"][g], "info": infos[g], "l2_lambda": lam}
               for g in range(H)]
        if wt:
            for g in range(H):
                out[g].update(kept=st["kept"][g], levels=len(st["scale"][g]))
        return out

    # ------------------------------------------------------------------ l2_lambda by blocked K-fold CV (ridge_lambda_grid)
    # DESIGN §5.3.6.  ridge_stats_begin(folds=K, block=b) keeps the sums per (head, fold); ridge_cv(grid) solves every fold's
    # training sums T_k = sum_{j != k} S_j for every lambda and scores the held-out fold from S_k's moments alone.
    def _ridge_stats_add_folds(self, st, cache, parts):
        """``ridge_stats_add`` with folds: each head's part of the chunk is partitioned on the host once more, by fold."""
        K, blk = st["folds"], st["block"]
        for g, ids, yy in parts:
            m = ids.numel()
            fold = (torch.arange(st["n"][g], st["n"][g] + m, dtype=torch.int64) // blk) % K
            for k in range(K):
                sel = torch.nonzero(fold == k).flatten()
                mk = sel.numel()
                if not mk:
                    continue
                yk = yy if mk == m else yy.index_select(0, sel.to(yy.device)).contiguous()
                self._ridge_accumulate(st, (g, k), cache, ids[sel], yk)
                if "tw" in st:
                    check(lib.vlb_ridge_sumsq_accumulate_masked(yk.data_ptr(), self.V, st["tw"][g].data_ptr(),
                                                                st["syy"][g, k].data_ptr(), mk, self.V, _stream()),
                          "vlb_ridge_sumsq_accumulate_masked")
                else:
                    check(lib.vlb_ridge_sumsq_accumulate(yk.data_ptr(), self.V, st["syy"][g, k].data_ptr(), mk, self.V, _stream()),
                          "vlb_ridge_sumsq_accumulate")
                st["n_fold"][g][k] += mk
            st["n"][g] += m

    def _ridge_fold_sums(self, st, g, skip):
        """(G, C, sz, sy) of head g summed over its folds but ``skip`` (-1: none), in ascending fold order, into the shared
        buffers st["T"] (the next call overwrites them; everything runs on one stream)."""
        K, E, V = st["folds"], self.E, self.V
        T = st.get("T")
        if T is None:
            f64, d = torch.float64, self.dev
            T = st["T"] = (torch.empty(E, E, dtype=f64, device=d), torch.empty(V, E, dtype=f64, device=d),
                           torch.empty(E, dtype=f64, device=d), torch.empty(V, dtype=f64, device=d))
        for name, out in zip(("G", "C", "sz", "sy"), T):
            check(lib.vlb_f64_sum_except(st[name][g].data_ptr(), out.numel(), K, int(skip), out.data_ptr(), out.numel(), _stream()),
                  "vlb_f64_sum_except")
        return T

    def ridge_cv(self, grid, per_target=False):
        """Blocked K-fold cross-validation of ``l2_lambda`` over ``grid`` from the per-fold sums: for every head g, fold k and
        grid point i the training sums T_k are solved (vlb_ridge_solve, N = N_g - n_gk) and the held-out fold is scored
        (vlb_ridge_cv_score) into an fp64 table [H,K,L,V] pre-filled with NaN.  Everything is queued without a host sync; the
        [H,K,L] infos and the table's target means are read once at the end.  The score of a grid point is the mean over heads
        and folds of the mean over targets of r; a grid point with any failed solve is excluded (a warning names it); the
        largest score wins and an exact tie goes to the larger lambda.  A (head, fold) with fewer than 2 clips, or every grid
        point excluded, raises.  The parameters are never written.  -> {"grid", "score" [L], "score_per_head" [H,L],
        "best_index", "best_lambda", "r" [H,L,V] (fold mean, on the device), "infos" [H][K][L]}.
        ``per_target=True`` also chooses one grid point per (head, target) on the device (vlb_ridge_cv_select,
        the same exclusions, a tie to the larger lambda) and adds "choice" [H,V] (device int32), "lambda_rows" [H,V] (device
        fp32, grid[choice]), "lambda_counts" [H][L] (one more device read) and "score_per_target", the mean over heads and
        targets of the winning fold-mean r - selected on the same folds it is scored on, so optimistic; everything else,
        "best_index" and "best_lambda" included, is what the call returns without it.
        With weighted stats every grid point is solved once per level with ``grid[i] * scale`` and scored into
        that level's targets (vlb_ridge_cv_score_rows); masked targets stay NaN in the table, every mean over targets is the plain
        mean over the kept ones, "infos" holds the first non-zero over the levels, and ``per_target`` chooses for kept targets
        only ("choice" -1 and "lambda_rows" = best_lambda at masked ones, "lambda_counts" counts kept targets)."""
        import warnings
        st = getattr(self, "_ridge", None)
        if st is None or "folds" not in st:
            raise RuntimeError("head: ridge_cv() needs ridge_stats_begin(folds=K) and the clips added")
        grid = self._ridge_grid("ridge_cv", grid)
        H, K, L, E, V, d = max(1, self.G), st["folds"], len(grid), self.E, self.V, self.dev
        name = self._head_name
        for g in range(H):
            for k in range(K):
                if st["n_fold"][g][k] < 2:
                    raise ValueError(f"head: ridge_cv: {name(g)}: fold {k} of {K} holds {st['n_fold'][g][k]} clip(s) (block = "
                                     f"{st['block']}, N = {st['n'][g]}): a held-out correlation needs 2 or more; use fewer folds or "
                                     "a smaller block")
        f64 = torch.float64
        A = torch.empty(E, E, dtype=f64, device=d)
        X = torch.empty(V, E, dtype=f64, device=d)
        W = torch.empty(V, E, dtype=torch.float32, device=d)        # vlb_ridge_solve's fp32 outputs: scratch here
        b = torch.empty(V, dtype=torch.float32, device=d)
        Gc = torch.empty(E, E, dtype=f64, device=d)
        Rc = torch.empty(V, E, dtype=f64, device=d)
        vy = torch.empty(V, dtype=f64, device=d)
        ws = torch.empty(lib.vlb_ridge_cv_ws_doubles(E, V), dtype=f64, device=d)
        table = torch.full((H, K, L, V), float("nan"), dtype=f64, device=d)
        wt = "tw" in st         # weighted stats (§5.3.9): per level one solve and a row-select score; masked targets stay NaN
        D = max(len(s) for s in st["scale"]) if wt else 1
        info = torch.zeros(H, K, L, D, dtype=torch.int32, device=d) if wt else torch.zeros(H, K, L, dtype=torch.int32, device=d)
        for g in range(H):
            for k in range(K):
                nk = st["n_fold"][g][k]
                Tg, Tc, Tsz, Tsy = self._ridge_fold_sums(st, g, k)
                check(lib.vlb_ridge_cv_center(st["G"][g, k].data_ptr(), st["C"][g, k].data_ptr(), st["sz"][g, k].data_ptr(),
                                              st["sy"][g, k].data_ptr(), st["syy"][g, k].data_ptr(), nk, Gc.data_ptr(), Rc.data_ptr(),
                                              vy.data_ptr(), E, V, _stream()), "vlb_ridge_cv_center")
                for i, lam in enumerate(grid):
                    if wt:
                        for lv, scale in enumerate(st["scale"][g]):
                            check(lib.vlb_ridge_solve(Tg.data_ptr(), Tc.data_ptr(), Tsz.data_ptr(), Tsy.data_ptr(), st["n"][g] - nk,
                                                      lam * scale, A.data_ptr(), X.data_ptr(), W.data_ptr(), b.data_ptr(),
                                                      info[g, k, i, lv:].data_ptr(), E, V, _stream()), "vlb_ridge_solve")
                            check(lib.vlb_ridge_cv_score_rows(X.data_ptr(), Gc.data_ptr(), Rc.data_ptr(), vy.data_ptr(),
                                                              ws.data_ptr(), table[g, k, i].data_ptr(),
                                                              info[g, k, i, lv:].data_ptr(), E, V, st["lvl"][g].data_ptr(), lv,
                                                              _stream()), "vlb_ridge_cv_score_rows")
                        continue
                    check(lib.vlb_ridge_solve(Tg.data_ptr(), Tc.data_ptr(), Tsz.data_ptr(), Tsy.data_ptr(), st["n"][g] - nk, lam,
                                              A.data_ptr(), X.data_ptr(), W.data_ptr(), b.data_ptr(), info[g, k, i:].data_ptr(), E, V,
                                              _stream()), "vlb_ridge_solve")
                    check(lib.vlb_ridge_cv_score(X.data_ptr(), Gc.data_ptr(), Rc.data_ptr(), vy.data_ptr(), ws.data_ptr(),
                                                 table[g, k, i].data_ptr(), info[g, k, i:].data_ptr(), E, V, _stream()),
                          "vlb_ridge_cv_score")
        infos = info.cpu()                              # the two device reads of the sweep
        if wt:      # [H,K,L]: the first non-zero over the levels; a level that failed leaves its targets NaN, so the mean is NaN
            first = (infos != 0).to(torch.int64).argmax(-1, keepdim=True)
            infos = infos.gather(-1, first).squeeze(-1)
            means = torch.stack([table[g].index_select(-1, st["kept_idx"][g]).mean(-1) for g in range(H)]).cpu()     # kept targets
        else:
            means = table.mean(-1).cpu()                # [H,K,L]; NaN where the solve failed
        ok = [not bool(infos[:, :, i].any()) for i in range(L)]
        for i in range(L):
            if not ok[i]:
                bad = [(g, k, int(infos[g, k, i])) for g in range(H) for k in range(K) if int(infos[g, k, i])]
                warnings.warn(f"head: ridge_cv: l2_lambda = {grid[i]!r} (grid point {i}) is excluded: "
                              + ", ".join(f"{name(g)} fold {k} info = {v}" for g, k, v in bad[:4])
                              + (" ..." if len(bad) > 4 else "") + " (a pivot that is not positive, or NaN / Inf in the targets)")
        if not any(ok):
            raise ValueError(f"head: ridge_cv: every grid point of {grid!r} had a failed solve; the parameters are unchanged")
        per_head = means.mean(1)                        # [H,L]
        score = per_head.mean(0)                        # [L]
        best = max((i for i in range(L) if ok[i]), key=lambda i: (float(score[i]), grid[i]))
        st["cv_table"] = table                          # [H,K,L,V], for inspection
        out = {"grid": grid, "score": [float(s) for s in score], "score_per_head": [[float(s) for s in row] for row in per_head],
               "best_index": best, "best_lambda": grid[best], "r": table.mean(1), "infos": infos.tolist()}
        if per_target:
            grid_d = torch.tensor(grid, dtype=f64, device=d)
            ok_d = torch.tensor([int(o) for o in ok], dtype=torch.int32, device=d)
            rmean = torch.empty(H, L, V, dtype=f64, device=d)
            choice = torch.empty(H, V, dtype=torch.int32, device=d)
            rbest = torch.empty(H, V, dtype=f64, device=d)
            for g in range(H):
                check(lib.vlb_ridge_cv_select(table[g].data_ptr(), grid_d.data_ptr(), ok_d.data_ptr(), rmean[g].data_ptr(),
                                              choice[g].data_ptr(), rbest[g].data_ptr(), K, L, V, _stream()), "vlb_ridge_cv_select")
            if wt:      # the choice is made for kept targets only: a masked one gets -1 / NaN and best_lambda in lambda_rows
                keep = st["keep"]
                choice = torch.where(keep, choice, torch.full_like(choice, -1))
                rbest = torch.where(keep, rbest, torch.full_like(rbest, float("nan")))
                idx = choice.to(torch.int64).clamp_(min=0)
                counts = torch.zeros(H, L, dtype=torch.int64, device=d).scatter_add_(1, idx, keep.to(torch.int64))
                packed = torch.cat([counts.to(f64).flatten(), rbest[keep].mean().reshape(1)]).cpu()  # the one device read
                lam_rows = torch.where(keep, grid_d.to(torch.float32)[idx],
                                       torch.full((), grid[best], dtype=f64, device=d).to(torch.float32))
            else:
                idx = choice.to(torch.int64)
                counts = torch.zeros(H, L, dtype=torch.int64, device=d).scatter_add_(1, idx, torch.ones_like(idx))
                packed = torch.cat([counts.to(f64).flatten(), rbest.mean().reshape(1)]).cpu()       # the one device read
                lam_rows = grid_d.to(torch.float32)[idx]
            st["cv_rmean"] = rmean                      # [H,L,V], for inspection
            out.update(choice=choice, lambda_rows=lam_rows, score_per_target=float(packed[-1]),
                       lambda_counts=[[int(c) for c in row] for row in packed[:-1].reshape(H, L)])
        return out

    def ridge_solve_rows(self, choice, grid):
        """The minimiser of the mse objective with one l2_lambda per target: ``choice`` int32 [H,V] on the
        device (``ridge_cv(per_target=True)``'s), ``grid`` its grid.  For every head and every grid point some target of that
        head chose, the head's totals are solved once with that lambda (vlb_ridge_solve_rows) and the rows that chose it are
        written into scratch; the infos are read once; a failed solve raises with the head, the grid point and the pivot named
        and leaves every parameter as it was.  Otherwise the fp32 masters and their bf16 copies are written as ``ridge_solve``
        writes them.  -> ``ridge_solve``'s list with "lambda_counts" [L] in place of "l2_lambda".
        With weighted stats ``choice`` may hold -1 at masked targets only; a kept target's code is
        choice * D + level, every used (grid point, level) is solved once with ``grid[i] * scale`` and masked rows are 0."""
        st = getattr(self, "_ridge", None)
        if st is None:
            raise RuntimeError("head: ridge_solve_rows() before ridge_stats_begin()")
        grid = self._ridge_grid("ridge_solve_rows", grid)
        H, E, V, L, d = max(1, self.G), self.E, self.V, len(grid), self.dev
        name = self._head_name
        if not isinstance(choice, torch.Tensor) or choice.dtype != torch.int32 or choice.numel() != H * V or \
                choice.device.type != torch.device(d).type:
            raise ValueError(f"head: ridge_solve_rows needs choice int32 [{H},{V}] on {d}")
        choice = choice.reshape(H, V).contiguous()
        for g in range(H):
            if st["n"][g] == 0:
                raise ValueError(f"head: ridge_solve_rows: {name(g)} has no clips (N = 0): nothing to fit it to")
        idx = choice.to(torch.int64)
        A = torch.empty(E, E, dtype=torch.float64, device=d)
        X = torch.empty(V, E, dtype=torch.float64, device=d)
        if "tw" in st:
            # weighted stats (§5.3.9): -1 at masked targets only; a kept target's code is choice * D + level, each used
            # (grid point, level) is solved once with grid[i] * scale and writes its rows into zeroed scratch
            keep, Dh = st["keep"], [len(s) for s in st["scale"]]
            if bool((keep & ((idx < 0) | (idx >= L))).any()) or bool((~keep & ((idx < -1) | (idx >= L))).any()):
                raise ValueError(f"head: ridge_solve_rows: choice holds an index outside [0, {L}) at a target with a positive "
                                 "weight (-1 is taken at masked targets only)")
            Dd = torch.tensor(Dh, dtype=torch.int32, device=d)[:, None]
            code = torch.where(keep, choice * Dd + st["lvl"], torch.full_like(choice, -1)).contiguous()
            Dmax = max(Dh)
            per = torch.zeros(H, L * Dmax + 1, dtype=torch.int64, device=d).scatter_add_(
                1, (code.to(torch.int64) + 1), torch.ones_like(idx))[:, 1:].tolist()
            counts = [[sum(per[g][i * Dh[g]:(i + 1) * Dh[g]]) for i in range(L)] for g in range(H)]
            used = [(g, i, lv) for g in range(H) for i in range(L) for lv in range(Dh[g]) if per[g][i * Dh[g] + lv]]
            W = torch.zeros(H, V, E, dtype=torch.float32, device=d)
            b = torch.zeros(H, V, dtype=torch.float32, device=d)
            info = torch.zeros(len(used), dtype=torch.int32, device=d)
            for j, (g, i, lv) in enumerate(used):
                Gs, Cs, szs, sys_ = self._head_totals(st, g)
                check(lib.vlb_ridge_solve_rows(Gs.data_ptr(), Cs.data_ptr(), szs.data_ptr(), sys_.data_ptr(), st["n"][g],
                                               grid[i] * st["scale"][g][lv], A.data_ptr(), X.data_ptr(), W[g].data_ptr(),
                                               b[g].data_ptr(), info[j:].data_ptr(), E, V, code[g].data_ptr(), i * Dh[g] + lv,
                                               _stream()), "vlb_ridge_solve_rows")
            used = [(g, i) for g, i, _ in used]
        else:
            if bool(((idx < 0) | (idx >= L)).any()):
                raise ValueError(f"head: ridge_solve_rows: choice holds an index outside [0, {L})")
            counts = torch.zeros(H, L, dtype=torch.int64, device=d).scatter_add_(1, idx, torch.ones_like(idx)).tolist()
            W = torch.empty(H, V, E, dtype=torch.float32, device=d)
            b = torch.empty(H, V, dtype=torch.float32, device=d)
            used = [(g, i) for g in range(H) for i in range(L) if counts[g][i]]
            info = torch.zeros(len(used), dtype=torch.int32, device=d)
            for j, (g, i) in enumerate(used):
                Gs, Cs, szs, sys_ = self._head_totals(st, g)
                check(lib.vlb_ridge_solve_rows(Gs.data_ptr(), Cs.data_ptr(), szs.data_ptr(), sys_.data_ptr(), st["n"][g], grid[i],
                                               A.data_ptr(), X.data_ptr(), W[g].data_ptr(), b[g].data_ptr(), info[j:].data_ptr(), E, V,
                                               choice[g].data_ptr(), i, _stream()), "vlb_ridge_solve_rows")
        infos = info.tolist()                           # the one device read of the solves
        for j, (g, i) in enumerate(used):
            if infos[j] < 0:
                raise ValueError(f"head: ridge_solve_rows: {name(g)}, l2_lambda = {grid[i]!r} (grid point {i}): target column "
                                 f"{-infos[j] - 1} holds a NaN or Inf (info = {infos[j]}, N = {st['n'][g]}); the parameters are "
                                 "unchanged")
            if infos[j]:
                raise ValueError(f"head: ridge_solve_rows: {name(g)}, l2_lambda = {grid[i]!r} (grid point {i}): pivot {infos[j]} "
                                 f"of {E} is not positive (info = {infos[j]}, N = {st['n'][g]}); the parameters are unchanged")
        self._write_ridge(W, b)
        return [{"subject": self.subjects[g] if self.G else None, "n": st["n"][g], "info": 0, "lambda_counts": counts[g]}
                for g in range(H)]

"""Frozen-backbone feature cache on the GPU: the cached head kernels against the uncached ones (bit for bit), and whole
fits with and without the cache (mini geometry, synthetic clips)."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("V", [1000, 2048])
@pytest.mark.parametrize("B", [3, 5])
def test_cached_head_step_is_bit_identical(dev, B, V):
    from phantom_vlb_amd._lib import check, lib
    from phantom_vlb_amd.feature_cache import FeatureCache
    from phantom_vlb_amd.head import BrainHead
    E, S, N = 4096, 96, 37
    gen = torch.Generator(device=dev).manual_seed(B * 7919 + V)
    head = BrainHead(E, V, 1e-3, 1e-5, dev, seed=B + V)
    for n in ("layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias"):
        head.master[n].add_(0.1 * torch.randn(E, generator=gen, device=dev))     # non-trivial affines
        head.compute[n].copy_(head.master[n])
    hidden = torch.randn(B, S, E, generator=gen, device=dev).mul_(2).add_(0.5).to(torch.bfloat16)
    wmask = torch.rand(B, S, generator=gen, device=dev)
    wmask[:, : S // 3] = 0                                            # zero-weight spans, as the prompt / padding have
    y = torch.randn(B, V, generator=gen, device=dev)
    keep = (torch.rand(B, E, generator=gen, device=dev) > 0.1).float() / 0.9
    cache = FeatureCache("train", N, E, dev)
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(B))[:B]         # permuted, scattered rows
    for ks in (None, keep):
        pred, terms = head.forward(hidden, wmask, y, ks)
        head.backward(need_dhidden=False)
        ref = (pred.clone(), terms.clone(), {n: g.clone() for n, g in head.grads.items()})
        ref_pr = (head.pooled_raw.clone(), head.sumw.clone())
        cache.store(idx, head)
        for t in (head.pooled_raw, head.sumw, head.zhat, head.ln2_rstd, head.pred, head.loss_terms, head.dz, head.dpooled):
            t.fill_(float("nan"))                                     # the cached step must produce all of them itself
        for g in head.grads.values():
            g.fill_(float("nan"))
        pred2, terms2 = head.forward_cached(cache, idx, y, ks)
        head.backward_cached()
        torch.cuda.synchronize()
        assert torch.equal(head.pooled_raw, ref_pr[0]) and torch.equal(head.sumw, ref_pr[1])
        assert torch.equal(pred2, ref[0]), "pred differs"
        assert torch.equal(terms2, ref[1]), "loss_terms differ"
        for n, g in head.grads.items():
            assert torch.equal(g, ref[2][n]), f"grad {n} differs"
        cache.valid[:] = False                                         # next round stores again (host bitmap only)
    # vlb_feature_cache_store: positions marked -1 write nothing, rows not named keep their values
    sentinel = -7.25
    cache.pooled.fill_(sentinel)
    cache.sumw.fill_(sentinel)
    rows = torch.full((B,), -1, dtype=torch.int32)
    rows[0], rows[B - 1] = 11, 36
    check(lib.vlb_feature_cache_store(head.pooled_raw.data_ptr(), head.sumw.data_ptr(), rows.to(dev).data_ptr(),
                                      cache.pooled.data_ptr(), cache.sumw.data_ptr(), B, E, N,
                                      torch.cuda.current_stream().cuda_stream), "store")
    torch.cuda.synchronize()
    assert torch.equal(cache.pooled[11], head.pooled_raw[0]) and torch.equal(cache.pooled[36], head.pooled_raw[B - 1])
    assert float(cache.sumw[11]) == float(head.sumw[0]) and float(cache.sumw[36]) == float(head.sumw[B - 1])
    others = [r for r in range(N) if r not in (11, 36)]
    assert bool((cache.pooled[others] == sentinel).all()) and bool((cache.sumw[others] == sentinel).all())
    # first write wins: a valid row is never overwritten by a later store
    cache.valid[:] = False
    cache.valid[11] = True
    before = cache.pooled[11].clone()
    head.pooled_raw.add_(1.0)
    assert cache.store(torch.tensor([11, 12] + [20 + i for i in range(B - 2)]), head) == B - 1
    torch.cuda.synchronize()
    assert torch.equal(cache.pooled[11], before) and torch.equal(cache.pooled[12], head.pooled_raw[1])


# ---------------------------------------------------------------------------------------------------- fits
def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.1, num_target=128, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8,
                weight_decay=1e-2, lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


def _dm():
    from phantom_vlb_amd.datamodule import VLBDataModule, VLBDataModuleConfig
    return VLBDataModule(VLBDataModuleConfig(lazyload_path="synthetic:3x8", subject="sub-99", seasons=["s1"], delay=3, window=3,
                                             random_state=1234, shuffle_val_data=False, batch_size=4, geometry="mini",
                                             num_target=128))


class _Rec:
    def __init__(self):
        self.rows = []

    def log_metrics(self, metrics, step):
        self.rows.append(dict(metrics))


def _fit(epochs=3, **kw):
    """VLB_mini_synthetic's loop (val_check_interval 0.5): what was logged, the head masters, and every backbone forward."""
    from phantom_vlb_amd.litmodule import VLBLitModule
    from phantom_vlb_amd.trainer import Trainer
    from src import LogValAccuracyCallback
    m = VLBLitModule(_cfg(**kw))
    m.configure_model()
    calls, phase, train_keys = [], ["?"], []
    fwd = m.backbone.forward
    m.backbone.forward = lambda *a, **k: (calls.append(phase[0]), fwd(*a, **k))[1]
    ts, vs = m.training_step, m.validation_step

    def training_step(batch):
        phase[0] = ("train", tr.current_epoch)
        train_keys.append((tr.current_epoch, set(batch)))
        return ts(batch)

    def validation_step(batch):
        phase[0] = ("val", tr.current_epoch)
        return vs(batch)
    m.training_step, m.validation_step = training_step, validation_step
    rec = _Rec()
    tr = Trainer(max_epochs=epochs, val_check_interval=0.5, log_every_n_steps=1, logger=rec,
                 callbacks=[LogValAccuracyCallback()])
    tr.fit(m, _dm())
    torch.cuda.synchronize()
    train = [r["train/brain_loss"] for r in rec.rows if "train/brain_loss" in r]
    val = [r["val/brain_loss"] for r in rec.rows if "val/brain_loss" in r]
    corr = [r["val_corr_avg"] for r in rec.rows if "val_corr_avg" in r]
    hit = [r for r in rec.rows if any(k.startswith("feature_cache/") for k in r)]
    return dict(train=train, val=val, corr=corr, masters={n: t.clone() for n, t in m.head.master.items()}, calls=calls,
                train_keys=train_keys, hit=hit, module=m)


@pytest.fixture(scope="module")
def padded_runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("fcache"))
    return _fit(pack_tokens=False), _fit(pack_tokens=False, cache_features=True, feature_cache_dir=d), d


def test_cached_fit_is_bit_identical_without_packing(padded_runs):
    ref, got, _ = padded_runs
    assert len(ref["train"]) == 12 and len(ref["val"]) == 6                  # 3 epochs x 4 batches, 2 passes per epoch
    assert got["train"] == ref["train"], (got["train"], ref["train"])
    assert got["val"] == ref["val"], (got["val"], ref["val"])
    assert got["corr"] == ref["corr"] and len(got["corr"]) == 6
    for n, t in ref["masters"].items():
        assert torch.equal(got["masters"][n], t), n
    # the backbone ran once per train batch of epoch 1 and once per val batch of the first pass, never again
    assert sorted(got["calls"]) == sorted([("train", 0)] * 4 + [("val", 0)] * 2), got["calls"]
    assert len(ref["calls"]) == 12 + 12
    assert all("vision" not in keys for ep, keys in got["train_keys"] if ep >= 1)
    assert all("vision" in keys for ep, keys in got["train_keys"] if ep == 0)
    rates = [r["feature_cache/train_hit_rate"] for r in got["hit"] if "feature_cache/train_hit_rate" in r]
    assert rates == [0.0, 1.0, 1.0]
    assert not ref["hit"]


def test_persisted_cache_is_reused_and_refused_on_another_seed(padded_runs):
    a, d = padded_runs[1], padded_runs[2]
    b = _fit(epochs=1, pack_tokens=False, cache_features=True, feature_cache_dir=d)
    assert b["calls"] == []                                                   # never calls the backbone
    assert b["train"] == a["train"][:4] and b["val"] == a["val"][:2]          # epoch 1, bit for bit
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        c = _fit(epochs=1, pack_tokens=False, cache_features=True, feature_cache_dir=d, init_seed=77)
    assert any("fingerprint mismatch" in str(x.message) for x in w)
    assert len(c["calls"]) == 4 + 2                                           # recomputed (and the files rewritten)
    assert c["train"] != a["train"][:4]


def test_cached_fit_with_packing_agrees_to_the_recorded_bound():
    ref = _fit(epochs=2)
    got = _fit(epochs=2, cache_features=True)
    rel = lambda a, b: max(abs(x - y) / abs(y) for x, y in zip(a, b))
    tr, va = rel(got["train"], ref["train"]), rel(got["val"], ref["val"])
    print(f"packed cached vs uncached: max rel train loss {tr:.3e}, val loss {va:.3e}")
    assert got["train"][:4] == ref["train"][:4]                 # epoch 1 computes the same features either way
    assert tr <= 1e-3 and va <= 1e-3            # measured: 0 on this geometry; 1e-3 if a tail plan moved with M

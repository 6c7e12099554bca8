"""GPU: the training-patch sampler (nsm_amd/patches.py, csrc/nsm_patch.hip)
against the numpy restatement of patch_util, bit for bit: the recorded draws,
the patches and the labels; flips with per-channel signs, the emitter offset,
the align grid, unaligned outputs, a pool beyond 2^31 elements, capture into a
graph, resume, the sampler in front of GraphedTrainStep, and from_dir."""
import functools
import json

import numpy as np
import pytest
import torch

import patch_util as U

pytestmark = pytest.mark.gpu

N, C, H, W = 5, 7, 37, 53
SENTINEL = -12345.0


def same_bits(a, b):
    a, b = torch.as_tensor(a).cpu().contiguous(), torch.as_tensor(b).cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=None)
def pool(E=1, n=N, h=H, w=W):
    """Seeded normal values with per-channel scales from 1e-2 to 1e3; each label
    plane is its own constant plus noise. Read-only: (inputs, labels, means, stds)."""
    rng = np.random.default_rng(20 + E)
    scale = np.logspace(-2, 3, C).astype(np.float32).reshape(1, C, 1, 1)
    x = (rng.standard_normal((n, C, h, w)).astype(np.float32) * scale + scale).astype(np.float32)
    y = (rng.random((n, E, h, w)).astype(np.float32) * 0.5
         + 10.0 * np.arange(E, dtype=np.float32).reshape(1, E, 1, 1)).astype(np.float32)
    means = x.astype(np.float64).mean(axis=(0, 2, 3)).astype(np.float32)
    stds = x.astype(np.float64).std(axis=(0, 2, 3)).astype(np.float32)
    for a in (x, y, means, stds):
        a.setflags(write=False)
    return x, y, means, stds


def make(device, E=1, **kw):
    import nsm_amd
    x, y, means, stds = pool(E)
    kw.setdefault("stats", (means.copy(), stds.copy()))
    kw.setdefault("record_draws", True)
    return nsm_amd.PatchSampler(torch.from_numpy(x.copy()).to(device),
                                torch.from_numpy(y.copy()).to(device), **kw)


def ref_draws(s, step):
    return U.draws(s.seed, s.rank, step, s.batch, frame=(s.H, s.W), patch=s.patch, lo=s.lo,
                   count=s.count, order=s.order, align=s.align, hflip=s.hflip, vflip=s.vflip,
                   emitters=s.E)


def ref_batch(s, step, E=1, stats=True, **kw):
    x, y, means, stds = pool(E)
    d = ref_draws(s, step)
    if stats:
        kw.update(means=means, stds=stds)
    return (d,) + U.gather(x, y, d, s.patch, **kw)


def check(s, step, got, **kw):
    d, rx, ry = ref_batch(s, step, **kw)
    assert np.array_equal(s.last_draws.cpu().numpy(), d), (step, s.last_draws.cpu(), d)
    assert same_bits(got[1], ry), f"labels of step {step}"
    assert same_bits(got[0], rx), f"patches of step {step}"
    return d


# ---- 1. the small pool ------------------------------------------------------------
@pytest.mark.parametrize("order", ["sequential", "random"])
@pytest.mark.parametrize("B", [3, 8])
@pytest.mark.parametrize("patch", [(16, 20), (37, 53), (15, 17), (8, 52)],
                         ids=lambda p: "x".join(map(str, p)))
def test_small_pool(device, patch, B, order):
    """Draws, patches and labels of three steps equal the restatement; without
    flips and emitter they also equal nsm_normalize_frames (the loader's kernel)
    applied to the whole pool and sliced by the recorded draws."""
    from nsm_amd._lib import call, ptr, stream
    s = make(device, patch=patch, batch=B, seed=1234, order=order, align=1)
    normed = s.inputs.clone()
    call("nsm_normalize_frames", ptr(normed), N, C, H * W, ptr(s.means), ptr(s.stds), U.EPS,
         stream())
    ph, pw = patch
    for step in range(3):
        x, y = s.next()
        assert x.requires_grad and x.dtype == torch.float32 and tuple(x.shape) == (B, C, ph, pw)
        assert tuple(y.shape) == (B, 1, ph, pw)
        d = check(s, step, (x.detach(), y))
        for i, (fr, oy, ox) in enumerate(d[:, :3].tolist()):
            assert same_bits(x[i].detach(), normed[fr, :, oy:oy + ph, ox:ox + pw])
            assert same_bits(y[i], s.labels[fr, :, oy:oy + ph, ox:ox + pw])
    if order == "sequential":
        assert s.last_draws[:, 0].tolist() == [(2 * B + i) % N for i in range(B)]


def test_no_stats_gives_raw_values(device):
    """stats=None: mean 0, std 1, eps 0, the pool's bits (a -0.0 included)."""
    s = make(device, patch=(16, 20), batch=4, seed=3, order="random", stats=None)
    s.inputs[:, :, ::3, ::5] = -0.0
    x, _ = s.next()
    for i, (fr, oy, ox) in enumerate(s.last_draws[:, :3].tolist()):
        assert same_bits(x[i].detach(), s.inputs[fr, :, oy:oy + 16, ox:ox + 20])


# ---- 2. flips, emitter, align -------------------------------------------------------
@pytest.mark.parametrize("patch", [(16, 20), (15, 17)], ids=lambda p: "x".join(map(str, p)))
def test_flips_with_channel_signs(device, patch):
    hs = [1.0, -1.0, 1.0, 1.0, -1.0, 1.0, 1.0]
    vs = [1.0, 1.0, -1.0, 1.0, 1.0, -1.0, 1.0]
    s = make(device, patch=patch, batch=64, seed=1234, order="random", hflip=True, vflip=True,
             hflip_sign=hs, vflip_sign=vs)
    d = ref_draws(s, 0)
    assert {(h, v) for h, v in d[:, 3:5].tolist()} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    check(s, 0, s.next(), hsign=hs, vsign=vs)
    # a mirrored normal channel is the negated mirror image of the plain crop
    x, _ = s.next()
    d = s.last_draws.cpu().numpy()
    i = int(np.flatnonzero((d[:, 3] == 1) & (d[:, 4] == 0))[0])
    fr, oy, ox = d[i, :3].tolist()
    xin, _, means, stds = pool()
    crop = xin[fr, 1, oy:oy + patch[0], ox:ox + patch[1]][:, ::-1]
    want = ((-crop - means[1]).astype(np.float32) / (stds[1] + np.float32(U.EPS))).astype(np.float32)
    assert same_bits(x[i, 1].detach(), want.copy())


def test_emitter_offset_and_label_plane(device):
    vals = [0.0, 1.0, 2.0, 3.0, 4.0]
    s = make(device, E=5, patch=(16, 20), batch=64, seed=1234, order="random", hflip=True,
             emitter_channel=5, emitter_values=vals)
    d = ref_draws(s, 0)
    assert set(d[:, 5].tolist()) == {0, 1, 2, 3, 4}
    x, y = s.next()
    check(s, 0, (x.detach(), y), E=5, emitter_channel=5, emitter_values=vals)
    # the label plane is the one of the drawn emitter: its constant is 10 e
    assert torch.equal((y.amin(dim=(1, 2, 3)) / 10).floor().cpu().int(), s.last_draws[:, 5].cpu())


def test_align_grid(device):
    s = make(device, patch=(16, 20), batch=8, seed=99, order="random", align=2)
    seen = []
    for step in range(4):
        d = check(s, step, tuple(t.detach() for t in s.next()))
        seen.append(d[:, 1:3])
    seen = np.concatenate(seen)
    assert (seen % 2 == 0).all() and seen[:, 0].max() <= 20 and seen[:, 1].max() <= 32
    assert len(np.unique(seen[:, 1])) > 4


# ---- 3. outputs ---------------------------------------------------------------------
def test_unaligned_destination(device):
    """out= views that start 4, 8 and 12 bytes past a 16-byte boundary (pw % 4 == 0
    would otherwise take the 16-byte stores): right values, nothing written
    outside."""
    s = make(device, patch=(16, 20), batch=3, seed=5, order="random", hflip=True)
    nx, ny = 3 * C * 16 * 20, 3 * 16 * 20
    for k, off in enumerate((1, 2, 3)):
        bx = torch.full((nx + 8,), SENTINEL, device=device)
        by = torch.full((ny + 8,), SENTINEL, device=device)
        x, y = bx[off:off + nx].view(3, C, 16, 20), by[off:off + ny].view(3, 1, 16, 20)
        assert x.data_ptr() % 16 == 4 * off
        rx, ry = s.next(out=(x, y))
        assert rx is x and ry is y
        check(s, k, (x, y))
        for buf, n in ((bx, nx), (by, ny)):
            assert (buf[:off] == SENTINEL).all() and (buf[off + n:] == SENTINEL).all()


def test_aligned_out_writes_nothing_else(device):
    s = make(device, patch=(8, 52), batch=3, seed=5, order="random")
    nx, ny = 3 * C * 8 * 52, 3 * 8 * 52
    bx = torch.full((nx + 8,), SENTINEL, device=device)
    by = torch.full((ny + 8,), SENTINEL, device=device)
    s.next(out=(bx[4:4 + nx].view(3, C, 8, 52), by[4:4 + ny].view(3, 1, 8, 52)))
    check(s, 0, (bx[4:4 + nx].view(3, C, 8, 52), by[4:4 + ny].view(3, 1, 8, 52)))
    for buf, n in ((bx, nx), (by, ny)):
        assert (buf[:4] == SENTINEL).all() and (buf[4 + n:] == SENTINEL).all()


@pytest.mark.parametrize("frames", [10, 40])
def test_large_pool(device, frames):
    """A pool of `frames` x 7 x 2048 x 4096 fp32 of which only the last frame is
    written: 10 frames are 2.35 GB (byte offsets beyond 2^31), 40 frames are
    2.3e9 elements (element offsets beyond 2^31). Sequential order over the
    one-frame shard of the last rank; no stats, so the patches are the slices."""
    import nsm_amd
    h, w = 2048, 4096
    try:
        inputs = torch.empty((frames, C, h, w), dtype=torch.float32, device=device)
        labels = torch.empty((frames, 1, h, w), dtype=torch.float32, device=device)
    except RuntimeError:
        free, total = torch.cuda.mem_get_info()
        pytest.skip(f"cannot allocate {frames * (C + 1) * h * w * 4 / 1e9:.1f} GB: "
                    f"{free / 1e9:.1f} of {total / 1e9:.1f} GB free")
    last = frames - 1
    g = torch.Generator(device=device).manual_seed(last)
    inputs[last] = torch.randn((C, h, w), device=device, generator=g)
    labels[last] = torch.rand((1, h, w), device=device, generator=g)
    s = nsm_amd.PatchSampler(inputs, labels, patch=(16, 20), batch=2, seed=1234, world=frames,
                             rank=last, record_draws=True)
    assert (s.lo, s.count) == (last, 1)
    x, y = s.next()
    d = ref_draws(s, 0)
    assert np.array_equal(s.last_draws.cpu().numpy(), d) and d[:, 0].tolist() == [last, last]
    assert d[0, 1:3].tolist() != d[1, 1:3].tolist()
    for i, (fr, oy, ox) in enumerate(d[:, :3].tolist()):
        assert same_bits(x[i].detach(), inputs[fr, :, oy:oy + 16, ox:ox + 20])
        assert same_bits(y[i], labels[fr, :, oy:oy + 16, ox:ox + 20])
    del s, inputs, labels, x, y
    torch.cuda.empty_cache()


# ---- 4. the stream --------------------------------------------------------------------
def test_capture_draws_a_new_batch_every_replay(device):
    s = make(device, patch=(16, 20), batch=3, seed=1234, order="random", hflip=True, vflip=True,
             capturable=True)
    x = torch.empty((3, C, 16, 20), device=device)
    y = torch.empty((3, 1, 16, 20), device=device)
    s.next(out=(x, y))                          # allocates the draw record outside the capture
    s.load_state_dict({"seed": 1234, "step": 5, "order": "random", "rank": 0})
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.next(out=(x, y))
    assert s.step == 5                          # a capture runs nothing
    seen = []
    for k in range(3):
        graph.replay()
        check(s, 5 + k, (x, y))
        seen.append((x.clone(), s.last_draws.clone()))
    assert s.step == 8
    for a in range(3):
        for b in range(a + 1, 3):
            assert not torch.equal(seen[a][0], seen[b][0])
            assert not torch.equal(seen[a][1], seen[b][1])


@pytest.mark.parametrize("capturable", [False, True], ids=["plain", "capturable"])
def test_resume(device, capturable):
    kw = dict(patch=(16, 20), batch=3, seed=2 ** 63 + 5, order="random", vflip=True,
              capturable=capturable)
    a = make(device, **kw)
    for _ in range(4):
        a.next()
    state = a.state_dict()
    assert state == {"seed": 2 ** 63 + 5, "step": 4, "order": "random", "rank": 0}
    want = [tuple(t.detach().clone() for t in a.next()) for _ in range(2)]
    b = make(device, **dict(kw, seed=0))
    b.load_state_dict(state)
    for k in range(2):
        got = tuple(t.detach() for t in b.next())
        assert same_bits(got[0], want[k][0]) and same_bits(got[1], want[k][1])
        check(b, 4 + k, got)
    assert b.state_dict() == dict(state, step=6)


def test_sampler_feeds_graphed_train_step(device):
    """Two GraphedTrainStep replays fed by sampler.next(out=(step.x, step.y))
    against two eager steps on the restatement's patches of the same steps:
    losses and state equal exactly, the tolerance of graph against eager in
    test_gpu_graph_step.py (`assert losses == ref` and the torch.equal loop
    below it, lines 47-49)."""
    import nsm_amd
    rng = np.random.default_rng(7)
    xin = rng.standard_normal((6, 7, 40, 48)).astype(np.float32)
    yin = rng.random((6, 1, 40, 48)).astype(np.float32)
    means, stds = xin.mean(axis=(0, 2, 3)), xin.std(axis=(0, 2, 3))

    def setup():
        torch.manual_seed(3)
        m = nsm_amd.Unet(in_ch=7, dropout_rate=0.0).to(device).train()
        opt = nsm_amd.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-3, max_grad_norm=1.0,
                                sanitize=True, seed=11)
        return m, opt, nsm_amd.CustomLoss(device, 0.9, vgg_weights=False)

    s = nsm_amd.PatchSampler(torch.from_numpy(xin).to(device), torch.from_numpy(yin).to(device),
                             patch=(32, 32), batch=2, stats=(means, stds), seed=1234, order="random",
                             hflip=True, record_draws=True)
    m, opt, crit = setup()
    g = torch.Generator(device=device).manual_seed(3)
    step = nsm_amd.GraphedTrainStep(m, crit, opt,
                                    torch.randn(2, 7, 32, 32, device=device, generator=g),
                                    torch.rand(2, 1, 32, 32, device=device, generator=g), warmup=1)
    losses = []
    for _ in range(2):
        s.next(out=(step.x, step.y))
        losses.append(step().item())
    m2, opt2, crit2 = setup()
    ref = []
    for t in range(2):
        d = U.draws(1234, 0, t, 2, frame=(40, 48), patch=(32, 32), lo=0, count=6, order="random",
                    hflip=True)
        rx, ry = U.gather(xin, yin, d, (32, 32), means=means, stds=stds)
        x, y = torch.from_numpy(rx).to(device), torch.from_numpy(ry).to(device)
        loss = crit2(m2(x), y, x)
        loss.backward()
        opt2.step()
        opt2.zero_grad()
        ref.append(loss.item())
    assert losses == ref, (losses, ref)
    assert torch.equal(opt.flat, opt2.flat)
    assert torch.equal(m.conv6.conv[0].weight, m2.conv6.conv[0].weight)


def test_from_dir_equals_tensor_constructor(device, tmp_path, monkeypatch):
    import nsm_amd
    from nsm_amd import patches
    monkeypatch.setattr(patches, "UPLOAD_BYTES", 4 * 4 * 4 * 24 * 40)   # batches of 4 and 2 frames
    rng = np.random.default_rng(11)
    xin = rng.standard_normal((6, 4, 24, 40)).astype(np.float32)
    yin = rng.random((6, 1, 24, 40))                                  # f64, as prepare_dataset writes
    means, stds = [0.1, -0.2, 0.3, 1.5], [1.0, 0.5, 2.0, 0.25]
    np.save(tmp_path / "train_inputs.npy", xin)
    np.save(tmp_path / "train_labels.npy", yin)
    (tmp_path / "train_stats.json").write_text(json.dumps({"means": means, "stds": stds}))
    kw = dict(patch=(16, 20), batch=4, seed=8, order="random", hflip=True, record_draws=True)
    a = nsm_amd.PatchSampler.from_dir(str(tmp_path), device=device, **kw)
    b = nsm_amd.PatchSampler(torch.from_numpy(xin).to(device),
                             torch.from_numpy(yin.astype(np.float32)).to(device),
                             stats=(means, stds), **kw)
    assert same_bits(a.inputs, b.inputs) and same_bits(a.labels, b.labels)
    for t in range(2):
        (xa, ya), (xb, yb) = a.next(), b.next()
        assert torch.equal(a.last_draws, b.last_draws)
        assert same_bits(xa.detach(), xb.detach()) and same_bits(ya, yb)
        d = U.draws(8, 0, t, 4, frame=(24, 40), patch=(16, 20), lo=0, count=6, order="random",
                    hflip=True)
        rx, ry = U.gather(xin, yin.astype(np.float32), d, (16, 20), means=means, stds=stds)
        assert same_bits(xa.detach(), rx) and same_bits(ya, ry)


def test_errors_raise_before_any_launch(device):
    with pytest.raises(ValueError, match="does not fit"):
        make(device, patch=(38, 16))
    with pytest.raises(ValueError, match="channels"):
        make(device, patch=(16, 16), stats=([0.0] * 4, [1.0] * 4))
    with pytest.raises(ValueError, match="emitter_values has 3"):
        make(device, E=5, patch=(16, 16), emitter_channel=5, emitter_values=[0.0, 1.0, 2.0])
    with pytest.raises(ValueError, match="go together"):
        make(device, patch=(16, 16), emitter_channel=5)
    s = make(device, patch=(16, 16), batch=2)
    with pytest.raises(ValueError, match="out x"):
        s.next(out=(torch.empty(2, C, 16, 20, device=device), torch.empty(2, 1, 16, 16, device=device)))
    assert s.step == 0 and s.last_draws is None

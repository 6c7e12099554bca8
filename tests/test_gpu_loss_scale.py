"""GPU, tail level: the device-side dynamic loss scaler (nsm_amd.GradScaler +
nsm_grad_tail_scaled, include/nsm.h) on injected gradients.

The contract is torch.amp.GradScaler's update rule (tests/loss_scale_util.py,
pinned to torch._amp_update_scale_ by tests/test_loss_scale_host.py), driven by
the tail's own census: found_inf = a NaN or Inf anywhere in the scaled gradient,
or a non-finite norm after the repair. Parameter sizes are those of
tests/test_gpu_optim_family.py (TAIL_CHUNK is 8192: a segment smaller than a
block, one crossing a block boundary, one exactly a block, a single element).

A note on the script's "norm > 1e5 after unscaling" step. The tail clips every
parameter's gradient to 1000*scale before it unscales (main.py:361-365), so the
unscaled norm the 1e5 check sees is never above ~1e3: the `huge` skip cannot
fire on a finite gradient, in the reference or here, and such a step is TAKEN
(oracle.step_tail_ref.sanitize_and_clip says so, and the test follows it). The
rule that a skip which is no overflow leaves the scale and the tracker alone is
therefore exercised with the other such skip, `postclip` (a clipped norm > 10,
main.py:408-418), reached by raising max_norm for that one step."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import loss_scale_util as U
from oracle.step_tail_ref import sanitize_and_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

SIZES = [5, 8192 + 3, 8192, 1]
OFFS = np.concatenate([[0], np.cumsum(SIZES)]).tolist()
TOTAL = OFFS[-1]
P_TOL = dict(rtol=1e-5, atol=2e-6)        # tests/test_gpu_tail.py's AdamW bounds
WD, LR, E = 1e-4, 1e-2, 200
BIG = 1 << 30                             # a growth interval never reached

# kind -> (flat class name, torch twin, optimizer keywords)
KINDS = {
    "adamw": ("FlatAdamW", torch.optim.AdamW, {}),
    "adam": ("FlatAdam", torch.optim.Adam, {}),
    "sgd": ("FlatSGD", torch.optim.SGD, {"momentum": 0.9}),
}


def _init(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in SIZES]


def _clean(seed, amp=1e-3):
    """A flat gradient of unscaled norm ~0.13 * amp/1e-3: below every threshold."""
    return torch.randn(TOTAL, generator=torch.Generator().manual_seed(seed)) * amp


def _seg(flat, i):
    return flat[OFFS[i]:OFFS[i + 1]]


def _build(kind, init, **kw):
    """(params, optimizer, flat gradient buffer the .grad views alias)."""
    import nsm_amd
    cls, _, okw = KINDS[kind]
    ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    opt = getattr(nsm_amd, cls)(ps, lr=LR, weight_decay=WD, max_grad_norm=1.0, sanitize=True,
                                seed=5, **okw, **kw)
    gflat = torch.zeros(TOTAL, device=DEV)
    for i, p in enumerate(ps):
        p.grad = _seg(gflat, i).view_as(p)
    return ps, opt, gflat


def _scaler(init_scale, policy="skip", interval=BIG, **kw):
    import nsm_amd
    return nsm_amd.GradScaler(init_scale=init_scale, growth_interval=interval, on_overflow=policy,
                              device=DEV, **kw)


def _snapshot(opt):
    """Everything the tail and the update kernel write, as host arrays."""
    torch.cuda.synchronize()
    ts = [opt.flat] + opt._moments() + [opt._step_dev[:1], opt.flags, opt.stat, opt._seg_coef]
    return [t.detach().cpu().numpy().copy() for t in ts]


def _same(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        # bitwise: compare the words, so that equal NaNs are equal
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), (what, k)


# ---- 1. the scaled tail is the static tail at an equal scale -----------------------
@pytest.mark.parametrize("kind,scale", [("adamw", 1.0), ("adamw", 2.0 ** 10), ("adamw", 2.0 ** 16),
                                        ("adam", 2.0 ** 10), ("sgd", 2.0 ** 10)])
def test_scaled_tail_is_bitwise_the_static_tail(kind, scale):
    init = _init()
    clean = _clean(11) * scale
    dirty = _clean(12) * scale
    _seg(dirty, 1)[17] = float("nan")
    _seg(dirty, 1)[8194] = float("inf")
    noise = torch.randn(TOTAL, generator=torch.Generator().manual_seed(13)).to(DEV)
    for policy in ("skip", "repair"):
        # the repaired gradient comes last: its backoff moves the scaler's scale
        grads = [clean, clean] + ([dirty] if policy == "repair" else [])
        _, ref, gref = _build(kind, init, grad_scale=scale)
        sc = _scaler(scale, policy)
        _, opt, g = _build(kind, init, grad_scaler=sc)
        for s, gr in enumerate(grads):
            gref.copy_(gr)
            g.copy_(gr)
            ref.step(noise=noise)
            opt.step(noise=noise)
            _same(_snapshot(opt), _snapshot(ref), (policy, s))
        assert ref.steps_taken() == opt.steps_taken() == len(grads)
        last = sc.last()
        assert last["scale"] == scale * (0.5 if policy == "repair" else 1.0)
        assert last["overflows"] == (1 if policy == "repair" else 0) and last["growths"] == 0
        assert not torch.equal(opt.flat.cpu(), torch.cat(init))         # it did step


# ---- 2. / 3. the scripted run --------------------------------------------------------
# step -> (what the gradient holds, max_norm of that step)
SCRIPT = [
    ("clean", 1.0), ("clean", 1.0), ("clean", 1.0),   # 0-2: a growth at step 2
    ("inf", 1.0),                                     # 3: one Inf in the 8195 segment
    ("clean", 1.0),                                   # 4
    ("nan1", 1.0),                                    # 5: a NaN in the size-1 segment (100 % of it)
    ("severe", 1.0),                                  # 6: 30 % of the 8192 segment invalid
    ("large", 1.0),                                   # 7: unscaled norm 1.8e5, finite: taken
    ("large", 100.0),                                 # 8: the same, max_norm 100: postclip skip
    ("clean", 1.0), ("clean", 1.0),                   # 9-10: the next growth at step 10
    ("clean", 1.0),                                   # 11
]
FOUND_INF = [0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 0, 0]
# "skip": every overflow is skipped; "repair": the tail repairs the single Inf of
# step 3 and steps (the static tail's decision), and skips the two severe ones
SKIPS = {"skip": [3, 5, 6, 8], "repair": [5, 6, 8]}
# the scale each step is taken at, from 1024 with growth_interval 3, and the
# tracker after it; the same under both policies, since the only step whose
# decision differs (3) is an overflow under both
SCALES = [1024, 1024, 1024, 2048, 1024, 1024, 512, 256, 256, 256, 256, 512]
TRACKERS = [1, 2, 0, 0, 1, 0, 0, 1, 1, 2, 0, 1]


def _script_grad(what, step, scale):
    if what == "large":
        return _clean(100 + step, 2e3) * scale
    g = _clean(100 + step) * scale
    if what == "inf":
        _seg(g, 1)[4321] = float("-inf")
    elif what == "nan1":
        _seg(g, 3)[0] = float("nan")
    elif what == "severe":
        idx = torch.randperm(SIZES[2], generator=torch.Generator().manual_seed(1))
        _seg(g, 2)[idx[:int(0.3 * SIZES[2])]] = float("nan")
    return g


def _run_script(kind, policy):
    """The scripted run on the device; after every step the scaler's state must
    equal the helper's replay. Returns per step (flags, scaler state, snapshot)."""
    sc = _scaler(1024.0, policy, interval=3)
    ps, opt, g = _build(kind, _init(), grad_scaler=sc)
    noise = torch.zeros(TOTAL, device=DEV)
    scale, tracker, overflows, growths, taken = 1024.0, 0, 0, 0, 0
    out = []
    for s, (what, max_norm) in enumerate(SCRIPT):
        assert scale == SCALES[s]
        g.copy_(_script_grad(what, s, scale))
        opt.max_grad_norm = max_norm
        before = _snapshot(opt)
        opt.step(noise=noise)
        fl, st, after = opt.last_flags(), sc.last(), _snapshot(opt)
        skipped = s in SKIPS[policy]
        new_scale, tracker = U.update(scale, tracker, FOUND_INF[s], 2.0, 0.5, 3,
                                      other_skip=skipped and not FOUND_INF[s])
        overflows += FOUND_INF[s]
        growths += new_scale > scale
        taken += not skipped
        assert st == dict(scale=new_scale, growth_tracker=tracker, found_inf=FOUND_INF[s],
                          overflows=overflows, growths=growths), (s, st)
        assert tracker == TRACKERS[s]
        assert fl["skip"] == int(skipped), (s, fl)
        assert opt.steps_taken() == taken
        if skipped:     # parameters, moments and the step count: bitwise untouched
            _same(after[:-3], before[:-3], f"skipped step {s}")
        out.append((fl, st, after))
        scale = new_scale
    assert opt.steps_taken() == len(SCRIPT) - len(SKIPS[policy])
    return out


@pytest.mark.parametrize("kind", list(KINDS))
def test_scripted_run_skip_policy(kind):
    got = _run_script(kind, "skip")
    # the decisions behind the skips
    assert got[5][0]["severe"] == 1 and got[6][0]["severe"] == 1
    assert got[3][0]["severe"] == 0 and got[3][0]["repaired"] == 1
    assert got[7][0]["huge"] == 0 and got[7][0]["postclip"] == 0      # see the module docstring
    assert got[8][0]["postclip"] == 1 and got[8][0]["huge"] == 0
    # the parameters: the torch optimizer stepped on the reference's sanitising
    # at the scale of each step, wherever a step is taken
    _, tw, okw = KINDS[kind]
    rps = [torch.nn.Parameter(t.clone()) for t in _init()]
    ropt = tw(rps, lr=LR, weight_decay=WD, foreach=False, **okw)
    worst = 0.0
    for s, (what, max_norm) in enumerate(SCRIPT):
        if FOUND_INF[s] or max_norm != 1.0:
            continue          # skipped by policy / the postclip step (max_norm is the test's)
        flat = _script_grad(what, s, float(SCALES[s]))
        for i, p in enumerate(rps):
            p.grad = _seg(flat, i).clone()
        assert not sanitize_and_clip(rps, 0, E, scale=float(SCALES[s])), s
        ropt.step()
        for i, r in enumerate(rps):
            a = got[s][2][0][OFFS[i]:OFFS[i + 1]]
            worst = max(worst, float(np.abs(a - r.detach().numpy()).max()))
            np.testing.assert_allclose(a, r.detach().numpy(), err_msg=f"step {s} p{i}", **P_TOL)
    print(f"{kind} scripted skip run: max |param - reference| = {worst:.3e}")


def test_scripted_run_repair_policy():
    """Steps are taken where the static tail takes them: the same script through
    a static-scale optimizer that is told each step's scale gives the same
    parameters, moments and flags bitwise. The scale trajectory is that of the
    skip policy (SCALES / TRACKERS): step 3 is an overflow under both."""
    got = _run_script("adamw", "repair")
    assert got[3][0]["repaired"] == 1 and got[3][0]["skip"] == 0
    _, ref, g = _build("adamw", _init())
    noise = torch.zeros(TOTAL, device=DEV)
    for s, (what, max_norm) in enumerate(SCRIPT):
        g.copy_(_script_grad(what, s, float(SCALES[s])))
        ref.grad_scale = float(SCALES[s])
        ref.max_grad_norm = max_norm
        ref.step(noise=noise)
        _same(got[s][2], _snapshot(ref), f"step {s}")
    assert ref.steps_taken() == len(SCRIPT) - len(SKIPS["repair"])


# ---- 4. the growth guard, and update(new_scale) ----------------------------------------
def test_growth_guard_and_explicit_update():
    sc = _scaler(2.0 ** 127, "skip", interval=1)
    _, opt, g = _build("adamw", _init(), grad_scaler=sc)
    g.copy_(_clean(3))                  # finite (an underflowing gradient at this scale)
    opt.step()
    st = sc.last()
    assert opt.last_flags()["skip"] == 0 and opt.steps_taken() == 1
    assert st == dict(scale=2.0 ** 127, growth_tracker=0, found_inf=0, overflows=0, growths=0)
    assert U.update(2.0 ** 127, 0, 0, 2.0, 0.5, 1) == (2.0 ** 127, 0)
    addr = sc.seed.data_ptr()
    assert addr == sc.state_tensor().data_ptr() and sc.seed.dim() == 0
    sc.update(new_scale=1024.0)
    assert sc.seed.data_ptr() == addr
    assert sc.get_scale() == 1024.0 and sc.last()["growth_tracker"] == 0
    assert float(sc.seed.item()) == 1024.0
    sc.update()                         # a no-op
    assert sc.get_scale() == 1024.0
    g.copy_(_clean(4) * 1024.0)
    opt.step()                          # interval 1: a growth
    assert sc.last() == dict(scale=2048.0, growth_tracker=0, found_inf=0, overflows=0, growths=1)


# ---- 5. checkpoints -------------------------------------------------------------------------
def test_state_dict_interchanges_with_torch():
    import nsm_amd
    sc = _scaler(4096.0, "skip", interval=7, growth_factor=4.0, backoff_factor=0.25)
    _, opt, g = _build("adamw", _init(), grad_scaler=sc)
    for s in range(2):
        g.copy_(_clean(s) * 4096.0)
        opt.step()
    sd = sc.state_dict()
    assert sd == {"scale": 4096.0, "growth_factor": 4.0, "backoff_factor": 0.25,
                  "growth_interval": 7, "_growth_tracker": 2}
    tsc = torch.amp.GradScaler("cpu")
    tsc.load_state_dict(sd)
    tsd = tsc.state_dict()
    assert tsd == sd and set(tsd) == set(sd)
    back = nsm_amd.GradScaler(device=DEV)
    addr = back.seed.data_ptr()
    back.load_state_dict(tsd)
    assert back.state_dict() == sd and back.seed.data_ptr() == addr
    assert back.tail_args()[:3] == (4.0, 0.25, 7)


def test_checkpoint_survives_a_backoff():
    sc = _scaler(1024.0, "skip", interval=3)
    ps, opt, g = _build("adamw", _init(), grad_scaler=sc)
    scale, tracker = 1024.0, 0
    for s, bad in enumerate([0, 0, 1, 0]):
        gr = _clean(20 + s) * scale
        if bad:
            _seg(gr, 1)[5] = float("inf")
        g.copy_(gr)
        opt.step()
        scale, tracker = U.update(scale, tracker, bad, 2.0, 0.5, 3)
    assert (scale, tracker) == (512.0, 1) and opt.steps_taken() == 3
    sc2 = _scaler(65536.0, "skip", interval=2000)
    sc2.load_state_dict(sc.state_dict())
    ps2, opt2, g2 = _build("adamw", [p.detach().cpu() for p in ps], grad_scaler=sc2)
    opt2.load_state_dict(opt.state_dict())
    nxt = _clean(30) * scale
    g.copy_(nxt)
    g2.copy_(nxt)
    opt.step()
    opt2.step()
    _same(_snapshot(opt2), _snapshot(opt), "resumed step")
    assert sc2.last()["scale"] == sc.last()["scale"] == 512.0
    assert sc2.last()["growth_tracker"] == sc.last()["growth_tracker"] == 2
    assert opt2.steps_taken() == 4


# ---- 6. capture -------------------------------------------------------------------------------
def test_scaled_tail_is_graph_capturable():
    """The tail alone under torch.cuda.graph: five replays across a backoff
    (step 1) and a growth (step 4, interval 3) equal five eager calls bitwise;
    one capture follows the moving scale."""
    runs = {}
    for capture in (False, True):
        sc = _scaler(1024.0, "skip", interval=3)
        _, opt, g = _build("adamw", _init(), grad_scaler=sc)
        graph = None
        if capture:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):        # recorded, not run
                opt.step()
        scale, tracker, trace = 1024.0, 0, []
        for s, bad in enumerate([0, 1, 0, 0, 0]):
            gr = _clean(40 + s) * scale
            if bad:
                _seg(gr, 2)[100] = float("inf")
            g.copy_(gr)                          # the gradient buffer is rewritten between replays
            graph.replay() if capture else opt.step()
            scale, tracker = U.update(scale, tracker, bad, 2.0, 0.5, 3)
            st = sc.last()
            assert (st["scale"], st["growth_tracker"]) == (scale, tracker), (capture, s, st)
            trace.append(_snapshot(opt) + [sc.state_tensor().cpu().numpy().copy()])
        assert scale == 1024.0 and st["overflows"] == 1 and st["growths"] == 1
        assert opt.steps_taken() == 4
        runs[capture] = trace
    for s, (a, b) in enumerate(zip(runs[False], runs[True])):
        _same(a, b, f"replay {s}")


# ---- 7. two ranks --------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, q):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "pcss-unet_amd"), os.path.join(ROOT, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sc = _scaler(1024.0, "skip", interval=2)
    _, opt, g = _build("adamw", _init(), grad_scaler=sc, world_size=world)
    res = []
    for s in range(3):        # an overflow on rank 1 only, then two clean steps (a growth)
        scale = [1024.0, 512.0, 512.0][s]
        gr = _clean(60 + 10 * s + rank) * scale
        if s == 0 and rank == 1:
            _seg(gr, 1)[8000] = float("inf")
        g.copy_(gr)
        dist.all_reduce(g)
        opt.step()
        torch.cuda.synchronize()
        res.append((opt.last_flags()["skip"], sc.last(), opt.flat.cpu().numpy().copy()))
    q.put((rank, opt.steps_taken(), res))      # by value: the worker exits right after
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_skip_together():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = dict((r[0], r[1:]) for r in (q.get(timeout=150) for _ in range(2)))
    finally:
        for p in procs:       # each child has its own limit; one past it is ended
            p.join(60)
            if p.is_alive():
                p.kill()
                p.join(30)
    for p in procs:
        assert p.exitcode == 0
    init = torch.cat(_init()).numpy()
    (taken0, r0), (taken1, r1) = res[0], res[1]
    assert taken0 == taken1 == 2
    for s in range(3):
        assert r0[s][0] == r1[s][0] == (1 if s == 0 else 0)
        assert r0[s][1] == r1[s][1]                                   # scale, tracker, counters
        assert np.array_equal(r0[s][2].view(np.int32), r1[s][2].view(np.int32))
    assert r0[0][1] == dict(scale=512.0, growth_tracker=0, found_inf=1, overflows=1, growths=0)
    assert np.array_equal(r0[0][2], init)                             # the skipped step
    assert not np.array_equal(r0[2][2], init)
    assert r0[2][1] == dict(scale=1024.0, growth_tracker=0, found_inf=0, overflows=1, growths=1)


# ---- 8. misuse raises ---------------------------------------------------------------------------------
def test_misuse_raises():
    import nsm_amd
    sc = _scaler(1024.0)
    ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in _init()]
    with pytest.raises(ValueError):
        nsm_amd.FlatAdamW(ps, sanitize=False, grad_scaler=sc)
    with pytest.raises(ValueError):
        nsm_amd.FlatAdamW(ps, sanitize=True, grad_scale=1024.0, grad_scaler=sc)
    with pytest.raises(ValueError):
        nsm_amd.make_optimizer(ps, "sgd", 1e-3, grad_scaler=sc)       # sanitize defaults to False
    opt = nsm_amd.make_optimizer(ps, "adamw", 1e-3, sanitize=True, grad_scaler=sc)
    other = nsm_amd.FlatAdamW([torch.nn.Parameter(torch.zeros(3, device=DEV))], sanitize=True)
    with pytest.raises(ValueError):
        sc.step(other)
    with pytest.raises(RuntimeError, match="tail"):
        sc.unscale_(opt)
    with pytest.raises(ValueError):
        _scaler(float("inf"))
    with pytest.raises(ValueError):
        sc.update(new_scale=0.0)
    # the right optimizer steps through the scaler
    for p in ps:
        p.grad = torch.zeros_like(p)
    sc.step(opt)
    sc.update()
    assert opt.steps_taken() == 1 and sc.last()["growth_tracker"] == 1
    assert opt.step_state()[-1] is sc.state_tensor()
    assert opt.step_hyper()[-1] == (2.0, 0.5, BIG, 1)

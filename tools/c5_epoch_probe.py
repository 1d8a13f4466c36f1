#!/usr/bin/env python3
"""GPU: what a training step on a freshly shuffled cigre14 + cigre14_reswitched mix (BASELINE C5) costs, on the C5 model, optimizer included:
  * the recorded mixed epoch (runner.EpochTrainer on MixedDataset.padded(): collation, structure rebuild and step replayed from one C call);
  * the eager epoch over DataLoader(MixedDataset) -- host-side composition, ragged collation, a new structure per batch -- in line and one
    batch ahead (PrefetchLoader);
  * the same step recorded on ONE resident batch: the floor.
A tree without the padded store (the parent of that feature) prints the last two.  `epoch` as argv[1]: only recorded epochs (for rocprofv3)."""
import importlib, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
pkg = importlib.import_module("deep-statistical-solver-for-distribution-system-state-estimation_amd")
REG = {"mu_v": 1e-1, "mu_theta": 1e-1, "lam_v": 1e-4, "lam_p": 1e-8, "lam_pf": 1e-6, "lam_reg": 1e2}
dev = torch.device("cuda:0")
B, S = int(os.environ.get("C5_B", "4096")), int(os.environ.get("C5_S", "8192"))
GRIDS = ["cigre14", "cigre14_reswitched"]
full = pkg.synthetic.make_batch(GRIDS, 256, seed=1)
parts = [pkg.dataset.DeviceDataset.from_batch(pkg.synthetic.make_batch([g], S, seed=2 + k, stats=full["stats"]), device=dev) for k, g in enumerate(GRIDS)]
ds = pkg.dataset.MixedDataset(parts)
st = tuple(s_.to(dev) for s_ in full["stats"])
H, L = (int(os.environ.get("C5_H", "256")), int(os.environ.get("C5_L", "8")))
steps_per_epoch = -(-len(ds) // B)


def fresh():
    torch.manual_seed(0)
    m = pkg.MPN(8, 6, 2, H, L, 2, 0.0).to(dev)
    return m, pkg.optim.FusedAdamax(m.parameters(), lr=3e-3, capturable=True)


def timed(fn, seconds=2.0, warm=1):
    """ms per call of fn() (which returns the number of steps it ran), host wall clock around device synchronisation."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        n += fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


print(f"C5 model MPN(8,6,2,{H},{L},2,0), B = {B}, {len(ds)} samples ({steps_per_epoch} steps per epoch), {torch.cuda.get_device_name(0)}")
t_rec = None
if hasattr(ds, "padded"):
    m, o = fresh()
    tr = pkg.runner.EpochTrainer(m, o, st, REG, ds.padded(), B, shuffle=True, mode=os.environ.get("C5_MODE", "plan"))

    def rec_epoch():
        tr.train_epoch()
        return steps_per_epoch
    if len(sys.argv) > 1 and sys.argv[1] == "epoch":
        for _ in range(10):
            rec_epoch()
        torch.cuda.synchronize(); sys.exit(0)
    t_rec = timed(rec_epoch)
    print(f"recorded mixed epoch ({tr.mode}, {tr.steps[B][0].n_launches if tr.mode == 'plan' else '?'} launches per step): {t_rec:.3f} ms/step")

# the floor: the same step recorded on one resident (unpadded) batch
m, o = fresh()
params = list(m.parameters())
bt = ds.collate(ds.ids[:B])
o.init_state()


def step_res():
    for p in params: p.grad = None
    out = m(bt.x[:, :8], bt.edge_index, bt.edge_attr[:, :6])
    loss = pkg.gsp_wls_edge(input=bt.x[:, :8], edge_input=bt.edge_attr[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2], edge_std=st[3],
                            edge_index=bt.edge_index, reg_coefs=REG, num_samples=None, node_param=bt.x[:, 8:], edge_param=bt.edge_attr[:, 6:])
    loss.backward(pkg.data.unit_grad(loss)); o.step(); return loss


plan = pkg.graphs.PlannedStep(step_res)


def res_steps():
    for _ in range(8): plan.replay()
    return 8
t_res = timed(res_steps)
print(f"resident batch, recorded step: {t_res:.3f} ms/step")
if t_rec is not None:
    print(f"recorded mixed epoch vs resident step: {100 * (t_rec / t_res - 1):+.1f} %")

gen = torch.Generator(); gen.manual_seed(0)
for name, wrap in [("in line", lambda l: l), ("PrefetchLoader", lambda l: pkg.dataset.PrefetchLoader(l))]:
    m, o = fresh()

    def eager_epoch():
        loader = wrap(pkg.dataset.DataLoader(ds, batch_size=B, shuffle=True, generator=gen))
        pkg.runner.train_epoch(m, o, loader, st, REG)
        return steps_per_epoch
    t = timed(eager_epoch)
    print(f"eager mixed epoch, {name}: {t:.3f} ms/step ({100 * (t / t_res - 1):+.1f} % vs resident)")

"""Held-out evaluation on the CPU: the synthetic test split, trainer.evaluate (single process and
gloo world size 2) and the trainers' --eval-size flag."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import torch

from torch_distributed_sandbox_amd.parallel import launch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "synthetic_train_seed0_first64.npz")


# ---------------------------------------------------------------- 8. the test split
def test_synthetic_train_split_is_unchanged_and_test_split_differs():
    from torch_distributed_sandbox_amd.data import SyntheticMNIST

    n = 600
    default = SyntheticMNIST(size=n)
    train = SyntheticMNIST(size=n, split="train")
    assert default.images.tobytes() == train.images.tobytes() and default.labels.tobytes() == train.labels.tobytes()
    # ... and those are the bytes the class produced before it had a split argument (recorded from it)
    gold = np.load(GOLDEN)
    assert gold["size"].item() == n
    assert default.images[:64].tobytes() == gold["images"].tobytes()
    assert default.labels.tobytes() == gold["labels"].tobytes()

    test = SyntheticMNIST(size=n, split="test")
    assert test.images.shape == train.images.shape and test.images.dtype == np.uint8
    assert not np.array_equal(test.labels, train.labels)  # a sample stream of its own
    assert (test.images != train.images).mean() > 0.5
    hist = np.bincount(test.labels, minlength=10)
    assert hist.sum() == n and len(hist) == 10
    # uniform labels: each class count is Binomial(600, 0.1), mean 60, sigma 7.3 -- 5 sigma either way
    assert hist.min() >= 60 - 37 and hist.max() <= 60 + 37, hist
    # the same templates: every class's mean test image correlates best with the mean train image
    # of that same class (the means differ by the averaged shifts and noise only)
    tr = np.stack([train.images[train.labels == c].mean(0).ravel() for c in range(10)])
    te = np.stack([test.images[test.labels == c].mean(0).ravel() for c in range(10)])
    corr = np.corrcoef(te, tr)[:10, 10:]  # [test class, train class]
    assert corr.argmax(1).tolist() == list(range(10)), corr.round(2)
    # deterministic
    assert SyntheticMNIST(size=50, split="test").images.tobytes() == SyntheticMNIST(size=50, split="test").images.tobytes()


# ---------------------------------------------------------------- 9. evaluate(), world size 2
H, N, BS = 32, 23, 5


def _model():
    from torch_distributed_sandbox_amd.models import ConvNet

    torch.manual_seed(0)
    m = ConvNet(image_shape=(H, H))
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():  # running statistics that matter
        for bn in (m.layer1[1], m.layer2[1]):
            bn.running_mean.copy_(0.2 * torch.randn(bn.num_features, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(bn.num_features, generator=g))
    return m


def _w_evaluate(rank, world, port, out_dir):
    from torch_distributed_sandbox_amd import trainer
    from torch_distributed_sandbox_amd.data import DeviceUpsampleLoader, SyntheticMNIST
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel, DistributedSampler
    from torch_distributed_sandbox_amd.parallel import distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model = DistributedDataParallel(_model())
    if rank != 0:  # a rank whose running statistics drifted: rank 0's are the authoritative ones
        with torch.no_grad():
            model.module.layer1[1].running_mean.add_(1.0)
            model.module.layer2[1].running_var.mul_(3.0)
    test = SyntheticMNIST(size=N, split="test")
    sampler = DistributedSampler(len(test), num_replicas=world, rank=rank, shuffle=False)
    loader = DeviceUpsampleLoader(test, BS, (H, H), "cpu", sampler=sampler, levels=True)
    model.train()
    ev = trainer.evaluate(model, loader, "cpu")
    assert model.module.training  # the previous mode is back
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(ev, f)
    dist.barrier()
    dist.destroy_process_group()


def test_evaluate_gloo_world2_counts_every_sample_once(tmp_path):
    from torch_distributed_sandbox_amd import trainer
    from torch_distributed_sandbox_amd.data import DeviceUpsampleLoader, SyntheticMNIST

    launch.spawn(_w_evaluate, args=(2, launch.find_free_port(), str(tmp_path)), nprocs=2, timeout=180)
    r0, r1 = (json.load(open(tmp_path / f"rank{r}.json")) for r in (0, 1))
    assert r0 == r1  # every rank returns the same dict
    assert r0["eval_samples"] == N  # 23 over 2 ranks: the sampler pads to 24, the padded sample is dropped
    model = _model()
    single = trainer.evaluate(model, DeviceUpsampleLoader(SyntheticMNIST(size=N, split="test"), BS, (H, H), "cpu",
                                                          levels=True), "cpu")
    assert single["eval_samples"] == N
    assert single["eval_accuracy"] == r0["eval_accuracy"]
    assert abs(single["eval_loss"] - r0["eval_loss"]) <= 1e-9 * abs(single["eval_loss"])  # (fp64 sums, another order)
    assert set(r0) == {"eval_loss", "eval_accuracy", "eval_samples", "eval_images_per_sec"}
    assert r0["eval_images_per_sec"] > 0


# ---------------------------------------------------------------- 10. the trainers' flag
def _run(args, timeout=300):
    e = dict(os.environ)
    e["CUDA_VISIBLE_DEVICES"] = ""  # CPU rehearsal even on a GPU box
    e["HIP_VISIBLE_DEVICES"] = ""
    return subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=e)


def test_mnist_onegpu_eval_size_flag():
    base = ["mnist_onegpu.py", "--device", "cpu", "--image-size", "32", "--epochs", "1", "--max-steps", "2",
            "--dataset-size", "50", "--json"]
    keys = {"eval_loss", "eval_accuracy", "eval_samples", "eval_images_per_sec"}
    p = _run(base + ["--eval-size", "12"])
    assert p.returncode == 0, p.stderr
    m = re.search(r"Test Accuracy: ([\d.]+) %, Test Loss: ([\d.]+) \((\d+) images\)", p.stdout)
    assert m is not None, p.stdout
    summ = json.loads(p.stdout.strip().splitlines()[-1])
    assert keys <= set(summ)
    assert summ["eval_samples"] == 12 and int(m.group(3)) == 12
    assert abs(float(m.group(1)) - 100.0 * summ["eval_accuracy"]) <= 0.005 + 1e-9
    assert abs(float(m.group(2)) - summ["eval_loss"]) <= 5e-5 + 1e-9
    assert 0.0 <= summ["eval_accuracy"] <= 1.0 and summ["eval_loss"] > 0
    assert p.stdout.index("Training complete in: ") < p.stdout.index("Test Accuracy: ")
    # without the flag: today's output
    q = _run(base)
    assert q.returncode == 0, q.stderr
    assert "Test Accuracy" not in q.stdout
    assert not (keys & set(json.loads(q.stdout.strip().splitlines()[-1])))

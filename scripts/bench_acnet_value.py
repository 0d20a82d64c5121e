"""k_acnet's value-head forms (MFAC forward with want_value, dense and with the Battle input support) timed alone on
262,144 random bench-shape rows, HIP-event median and minimum of 10: the forms scripts/bench_policy.py does not reach.

    python scripts/bench_acnet_value.py"""
import json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mean-field-multi-agent-reinforcement-learning_amd", "python"))
import numpy as np
import torch
from mfrl_amd.algo.nets import ACNet
from mfrl_amd.policy import ACNetHIP
torch.cuda.set_device(0)
torch.manual_seed(3)
n, reps = 262144, 10
view = torch.rand((n, 13, 13, 7), device="cuda")
feat = torch.rand((n, 34), device="cuda")
prob = torch.rand((n, 21), device="cuda")
net = ACNet((13, 13, 7), (34,), 21, use_mf=True).cuda()
out = {}
for support in (False, True):
    hip = ACNetHIP((13, 13, 7), (34,), 21, True).load(net)
    v = view
    if support:
        y, x = np.mgrid[-6:7, -6:7]
        circle = (x * x + y * y <= 36)[:, :, None]
        mask = (circle | (np.arange(7) % 3 == 0)[None, None, :] & (np.arange(7) > 0)[None, None, :]).reshape(-1)
        v = view * torch.from_numpy(mask.astype(np.float32).reshape(13, 13, 7)).cuda()
        hip.set_input_support(mask.astype(np.uint8))
    run = lambda k: hip.forward(v, feat, prob, want_policy=False, want_value=True, seed=1, step=k)
    for k in range(2):
        run(k)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for k in range(reps):
        ev[k][0].record(); run(k); ev[k][1].record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    out["support" if support else "dense"] = {"ms_median": ms[len(ms) // 2], "ms_min": ms[0]}
print(json.dumps({"net": "acnet_mf_value", "n": n, **out}), flush=True)

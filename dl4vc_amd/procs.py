"""One child process per GPU: what ``main.py --gpus N`` and ``tools/candidate_generator.py --gpus N`` share."""
from __future__ import annotations

import os
import time


def child_devices(n: int):
    """HIP_VISIBLE_DEVICES value of each of the ``n`` shard processes: the g-th entry of the PARENT's device mask
    (HIP_VISIBLE_DEVICES, else CUDA_VISIBLE_DEVICES, which HIP honours too), or plain g without a mask.  A
    ROCR_VISIBLE_DEVICES mask needs no handling: HIP indices are already relative to it and the children inherit it."""
    if os.environ.get("DL4VC_FORCE_DEVICE0"):                 # rehearse the multi-process path on a one-GPU box (tests)
        return ["0"] * n
    mask = os.environ.get("HIP_VISIBLE_DEVICES", os.environ.get("CUDA_VISIBLE_DEVICES"))
    if mask is None:
        return [str(g) for g in range(n)]
    have = [d.strip() for d in mask.split(",") if d.strip()]
    if len(have) < n:
        raise SystemExit("--gpus %d but the device mask '%s' lists only %d device(s)" % (n, mask, len(have)))
    return have[:n]


def child_env(device: str, **extra) -> dict:
    """The environment of the shard process on ``device`` (an entry of ``child_devices``)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES=device, HSA_ENABLE_IPC_MODE_LEGACY="0", **extra)
    env.pop("CUDA_VISIBLE_DEVICES", None)                     # (HIP honours both; the mask is carried in HIP_VISIBLE_DEVICES)
    return env


def wait_children(procs, poll_s: float = 0.2):
    """Return codes of the child processes; as soon as ONE exits non-zero the others are terminated (a rank that died leaves
    its siblings blocked in a collective until the backend's timeout -- and a parent waiting on them in rank order blocked
    with them)."""
    rcs = [None] * len(procs)
    failed = False
    while any(rc is None for rc in rcs):
        for i, p in enumerate(procs):
            if rcs[i] is None:
                rcs[i] = p.poll()
        if not failed and any(rc not in (None, 0) for rc in rcs):
            failed = True
            for i, p in enumerate(procs):
                if rcs[i] is None:
                    p.terminate()
            deadline = time.time() + 20.0
            while time.time() < deadline and any(p.poll() is None for p in procs):
                time.sleep(poll_s)
            for p in procs:
                if p.poll() is None:
                    p.kill()
        if any(rc is None for rc in rcs):
            time.sleep(poll_s)
    return rcs

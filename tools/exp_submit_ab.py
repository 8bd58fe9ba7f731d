#!/usr/bin/env python3
"""
The headline loop of bench.py (VGG-16 predict_async, 600x1000, N images in flight on the slot streams) with the model attribute
bench.py cannot pass: --native-submit 1 (frcnn_predict_submit: dependency on the producer only when it is busy, one packed D2H copy) or 0
(the Python sequence wait_stream -> forward -> detections -> three copies -> record).  Prints one JSON line: images/sec of the median burst,
every burst, the dependencies taken / skipped over all slots, and which slot streams share a hardware queue with the default stream or
with each other (frcnn_streams_share_queue).  Run both settings in turn, in the environment to be judged (GPU_MAX_HW_QUEUES as set):

    python tools/exp_submit_ab.py --native-submit 0; python tools/exp_submit_ab.py --native-submit 1
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--native-submit", type=int, default=1, choices=[0, 1])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--pool", type=int, default=8)
    ap.add_argument("--ramp-seconds", type=float, default=2.0)
    ap.add_argument("--min-timed-seconds", type=float, default=2.0)
    args = ap.parse_args()

    from fasterrcnn_amd import _native as nv, runtime as rt, synthetic
    from fasterrcnn_amd.models.faster_rcnn import FasterRCNNModel
    from fasterrcnn_amd.models.vgg16 import VGG16Backbone
    nv.require_gpu()
    dev = torch.device("cuda", 0)
    model = FasterRCNNModel(num_classes=21, backbone=VGG16Backbone(dropout_probability=0.0))
    model.load_state_dict(synthetic.vgg16_state_dict(1234), strict=True)
    model = model.cuda(dev).eval()
    model.native_submit = bool(args.native_submit)
    pool = [synthetic.image(s).unsqueeze(0).to(dev) for s in range(args.pool)]
    n = max(1, args.inflight)

    def run(steps):
        pending = []
        for i in range(steps):
            if len(pending) == n:
                pending.pop(0).result()
            pending.append(model.predict_async(pool[i % len(pool)], 0.05, slot=0 if n == 1 else 1 + (i % n)))
        while pending:
            pending.pop(0).result()

    t_ramp = time.perf_counter() + args.ramp_seconds
    while time.perf_counter() < t_ramp:
        run(n)
    run(max(args.warmup, n))
    bursts, total = [], 0.0
    while not bursts or (total < args.min_timed_seconds and len(bursts) < 64):
        torch.cuda.synchronize(dev)
        ts = time.perf_counter()
        run(args.steps)
        torch.cuda.synchronize(dev)
        bursts.append(time.perf_counter() - ts)
        total += bursts[-1]
    srt = sorted(bursts)
    taken = skipped = 0
    for slot in model._slots.values():
        a, b = C.c_int64(), C.c_int64()
        nv.check(nv.lib().frcnn_ctx_submit_stats(slot.ctx.handle, C.byref(a), C.byref(b)), "frcnn_ctx_submit_stats")
        taken, skipped = taken + a.value, skipped + b.value
    streams = {"default": torch.cuda.default_stream(dev)}
    streams.update({"slot%d" % i: rt.slot_stream(dev, i) for i in range(1, n + 1)} if n > 1 else {})
    names = list(streams)
    shared = [[x, y] for i, x in enumerate(names) for y in names[i + 1:] if rt.streams_share_queue(streams[x], streams[y])]
    q = os.environ.get("GPU_MAX_HW_QUEUES")
    print(json.dumps({"native_submit": bool(args.native_submit), "hip_hw_queues": int(q) if q else None, "inflight": n,
                      "value": round(args.steps / srt[(len(srt) - 1) // 2], 3), "unit": "images/sec",
                      "bursts": [round(args.steps / b, 1) for b in bursts], "dependencies_taken": taken, "dependencies_skipped": skipped,
                      "streams_sharing_a_queue": shared, "streams_passed_over": len(rt._passed_over_streams)}), flush=True)


if __name__ == "__main__":
    main()

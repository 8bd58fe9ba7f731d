"""
bench.py -- images/sec of Faster R-CNN VGG-16 inference (600x1000, 300 proposals) on N x MI355X.

  python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W

A plain run measures the headline alone: it sets up, warms up, times the K steps, writes --dump-outputs and prints the line.
Everything else this file measures or checks runs only with `--full`: the other arithmetic tables, the host-fed, single-stream,
ResNet-50 and train-step legs, the per-rank burst, clocks under load, the parity block, the host CPU per image, mAP@0.5, the
roofline block and the CPU baseline.  Their fields are null (or absent) in a plain run's line.

A "step" is one `predict()` of one synthetic, already-preprocessed float32 3x600x1000 image that is
resident in HBM when the timed region starts: VGG-16 backbone, RPN (6000 pre- / 300 post-NMS),
RoI pooling, FC head, on-device float64 decode + per-class NMS, one D2H copy of the detections.
Every image is an independent batch-1 forward (BASELINE.json configs[1]); `--inflight` of them (default 4)
are in flight on separate HIP streams (with as many HIP hardware queues as the environment gives the process).  float32 tensors end to end (the
reference's dtype).  WHICH matrix instructions every GEMM-shaped layer runs on is part of the JSON line (`dtype`, `layer_arithmetic`,
`fc_math`, `winograd_x6_layers`, `winograd_x3_layers`, `f32_pipe_tflops` / `bf16_pipe_tflops` / `f16_pipe_tflops`): the 3x3 convolutions
up to conv3_3 on the exact-f32 MFMA pipe as one-launch Winograd F(2x2,3x3) layers (`math`); the 512-channel layers (conv4_1 ... conv5_3,
RPN trunk) as Winograd layers whose GEMMs run in the "f32x3" split-operand arithmetic, as do fc1 / fc2 (two fp16 terms per block-scaled
operand, three fp16 MFMAs per product, f32 accumulation: operands held to 22-23 bits of their row's / tile's largest element); the 1x1 /
head GEMMs on the exact-f32 pipe.  The table is chosen by measurement against a float64 evaluation of the network on held-out images
(the f32x3 layers are CLOSER to the float64 truth than the exact-f32 matrix instructions are).  Legs of the same
workload in the same run (--full): `config.strict_f32_images_per_sec` (EVERY GEMM on the exact-f32 pipe), `config.h2d_preprocess_images_per_sec`
(fed from pinned host memory through H2D + GPU preprocessing inside the timed region), `fc_math_f32_images_per_sec`,
`winograd_all_f32_pipe_images_per_sec`, `f32x6_only_images_per_sec`, `round3_table_images_per_sec`.

Multi-GPU: image-parallel, rank r owns its own images, no data-path collective; weak scaling
(K steps per rank).  With --full, the mAP@0.5 bookkeeping runs after the timed region on a small labelled
subset and is merged across ranks with the single all-gather of fasterrcnn_amd/evaluate.py.

The headline is ONE timed burst of exactly K steps (`--min-timed-seconds S` repeats it until S seconds are timed and reports
the median burst); `ms_per_step` is that burst's milliseconds per step.  `--dump-outputs DIR` writes what the last timed step
returned -- predict()'s per-class (n, 5) float64 detections -- as DIR/detections.npy, (N, 6) rows of (class, y1, x1, y2, x2,
score) in class order, plus DIR/detections_per_class.npy, the row count of each class (rank 0; the inputs are seeded, so the
same flags give the same inputs on every run and two builds can be compared output for output).  `config.hip_hw_queues` is the
GPU_MAX_HW_QUEUES the environment sets, or null when it is unset (the HIP runtime's own default applies; bench.py sets none).

Prints ONE JSON line on rank 0 (see DESIGN.md section "Measurement" for every field).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402
import torch.distributed as dist   # noqa: E402

H, W = 600, 1000
PEAK_F32_MFMA_TFLOPS = 157.3     # /opt/skills/guides/MI355X_MICROARCH.md, "Peak FP32 (matrix)"
PEAK_BF16_MFMA_TFLOPS = 2500.0   # same table, "Peak BF16/FP16 MFMA" dense (never the 2:1-sparsity figure)
PEAK_HBM_GBS = 8000.0            # same guide: HBM3E ~8 TB/s

# (cin, cout, h, w) of the 3x3 convolutions that run on the MFMA kernel (conv1_1 is the VALU kernel)
_MFMA_CONVS = [(64, 64, 600, 1000), (64, 128, 300, 500), (128, 128, 300, 500), (128, 256, 150, 250),
               (256, 256, 150, 250), (256, 256, 150, 250), (256, 512, 75, 125), (512, 512, 75, 125),
               (512, 512, 75, 125), (512, 512, 37, 62), (512, 512, 37, 62), (512, 512, 37, 62),
               (512, 512, 37, 62)]   # last = RPN trunk (models/rpn.py:88)


_CONV_NAMES = ["conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3", "conv5_1", "conv5_2",
               "conv5_3", "rpn_trunk"]


def uses_winograd(cin, cout):       # fasterrcnn_amd/_native.py uses_winograd_fused: every single-map 3x3 layer from conv1_2 on
    return cin >= 64 and cin % 16 == 0 and cout >= 64 and cout % 64 == 0


def conv_mfma_flops_per_image():
    return float(sum(2.0 * 9 * ci * co * h * w for ci, co, h, w in _MFMA_CONVS))


_POOLED = ("conv1_2", "conv2_2", "conv3_3", "conv4_3")       # layers with the fused 2x2 max-pool (models/vgg16.py:79,82,86,90)


def direct_layers(math, x6=()):
    """The 3x3 layers that run on conv3x3_mfma_kernel in this math mode."""
    return [l for n, l in zip(_CONV_NAMES, _MFMA_CONVS) if not (math == "f32_winograd" and (uses_winograd(l[0], l[1]) or n in x6))]


def winograd_layers(math, x6=(), named=False, x3f=()):
    """The layers that run as one-launch float32 Winograd layers (wino_fused_kernel, exact-f32 pipe)."""
    out = [(n, l) for n, l in zip(_CONV_NAMES, _MFMA_CONVS) if math == "f32_winograd" and uses_winograd(l[0], l[1]) and n not in x6 and n not in x3f]
    return out if named else [l for _, l in out]


def x3f_winograd_layers(math, x6=(), x3f=()):
    """The layers that run as ONE-launch f32x3 Winograd layers (csrc/wino_x3f.hip: wino_x3d_kernel, fp16 pipe), named."""
    return [(n, l) for n, l in zip(_CONV_NAMES, _MFMA_CONVS) if math == "f32_winograd" and n in x3f and n not in x6]


def x6_winograd_layers(math, x6=(), named=False):
    """The layers that run as x6 Winograd layers (csrc/wino_x6.hip: gemm_x6t_kernel on the bf16 pipe)."""
    out = [(n, l) for n, l in zip(_CONV_NAMES, _MFMA_CONVS) if math == "f32_winograd" and n in x6]
    return out if named else [l for _, l in out]


def winograd_gemm_flops(ci, co, h, w):
    """FLOP the matrix pipe executes for one Winograd F(2x2,3x3) layer: 16 positions x tiles x cin x cout x 2 (tiles = the image's
    ceil(h/2) x ceil(w/2); the padding of the kernel's 2 x 16-tile blocks is NOT counted -- it is waste, not work)."""
    return 2.0 * 16 * ((h + 1) // 2) * ((w + 1) // 2) * ci * co


def layer_arithmetic(math, fc_math, x6=(), n_rois=300, num_classes=21, x3=(), x3f=()):
    """One row per GEMM-shaped layer of one image: which kernel family and WHICH matrix pipe it runs on, the FLOP that pipe executes
    for it and the algorithmic (direct-form) FLOP it stands for.  Winograd layers execute 16 x tiles x cin x cout x 2; an "x6" layer
    executes six bf16 MFMAs per algorithmic product, an "x3" layer (a subset of the x6 table) three fp16 MFMAs."""
    rows = []
    for name, (ci, co, h, w) in zip(_CONV_NAMES, _MFMA_CONVS):
        alg = 2.0 * 9 * ci * co * h * w
        if math == "f32_winograd" and name in x3f and name not in x6:
            rows.append((name, "wino_x3d_kernel (one-launch x3 Winograd layer)", "f16", 3.0 * winograd_gemm_flops(ci, co, h, w), alg))
        elif math == "f32_winograd" and name in x6 and name in x3:
            rows.append((name, "gemm_x3t_kernel (x3 Winograd layer)", "f16", 3.0 * winograd_gemm_flops(ci, co, h, w), alg))
        elif math == "f32_winograd" and name in x6:
            rows.append((name, "gemm_x6t_kernel (x6 Winograd layer)", "bf16", 6.0 * winograd_gemm_flops(ci, co, h, w), alg))
        elif math == "f32_winograd" and uses_winograd(ci, co):
            rows.append((name, "wino_fused_kernel", "f32", winograd_gemm_flops(ci, co, h, w), alg))
        else:
            rows.append((name, "conv3x3_mfma_kernel", "f32", alg, alg))
    alg = 2.0 * 512 * 45 * 37 * 62
    rows.append(("rpn_heads_1x1", "linear_mfma_kernel", "f32", alg, alg))
    for name, k, n in (("fc1", 25088, 4096), ("fc2", 4096, 4096)):
        alg = n_rois * 2.0 * k * n
        if fc_math == "f32x3":
            rows.append((name, "gemm_x3t_kernel", "f16", 3.0 * alg, alg))
        elif fc_math == "f32x6":
            rows.append((name, "gemm_x6t_kernel", "bf16", 6.0 * alg, alg))
        else:
            rows.append((name, "linear_mfma_kernel", "f32", alg, alg))
    alg = n_rois * 2.0 * 4096 * (5 * num_classes - 4)
    rows.append(("detector_heads", "linear_mfma_kernel", "f32", alg, alg))
    return rows


def pipe_flops_per_image(math, fc_math, x6=(), backbone_only=False, x3=(), x3f=()):
    """FLOP each matrix pipe executes per image: {"f32": exact-f32 MFMAs, "bf16": bf16 MFMAs (f32x6 layers), "f16": fp16 MFMAs (f32x3 layers)};
    bf16 and fp16 instructions run at the same dense peak."""
    out = {"f32": 0.0, "bf16": 0.0, "f16": 0.0}
    for name, _, pipe, ex, _ in layer_arithmetic(math, fc_math, x6, x3=x3, x3f=x3f):
        if backbone_only and not (name.startswith("conv") or name == "rpn_trunk"):
            continue
        out[pipe] += ex
    return out


def executed_mfma_flops_per_image(math, fc_math="f32", x6=(), x3=(), x3f=()):
    """Matrix-pipe FLOP executed per image, all pipes added (kept for continuity with rounds 1-2; the per-pipe figures are the meaningful ones)."""
    f = pipe_flops_per_image(math, fc_math, x6, x3=x3, x3f=x3f)
    return f["f32"] + f["bf16"] + f["f16"]


def total_flops_per_image(n_rois=300):
    conv1_1 = 2.0 * 27 * 64 * H * W
    rpn_heads = 2.0 * 512 * 45 * 37 * 62
    det = n_rois * 2.0 * (25088 * 4096 + 4096 * 4096 + 4096 * 101)
    return conv1_1 + conv_mfma_flops_per_image() + rpn_heads + det


def measured_traffic(family="conv3x3_mfma_kernel"):
    """HBM bytes per launch of a kernel family from the newest committed PMC passes (profiles/rNN/traffic.json:
    FETCH_SIZE and WRITE_SIZE collected in separate rocprofv3 runs, FETCH_SIZE doubled per the gfx950
    note in MI355X_MICROARCH.md).  bench.py cannot run rocprofv3 on itself, so this is the recorded value."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "traffic.json")))
    if not files:
        return None
    try:
        rec = json.load(open(files[-1]))
        # staleness guard: the recorded kernel must still exist in the library that is being benchmarked (a renamed or removed
        # kernel returns None instead of a number measured on code that no longer runs)
        from fasterrcnn_amd import _native
        if family.encode() not in open(_native.LIB_PATH, "rb").read():
            return None
        if "by_kernel" in rec:
            return float(rec["by_kernel"][family]["hbm_bytes_per_launch"]) if family in rec["by_kernel"] else None
        return float(rec["hbm_bytes_per_launch"]) if family == "conv3x3_mfma_kernel" else None
    except Exception:
        return None


def profiled_launch_us(family):
    """Mean launch duration (us) of a kernel family in the newest COMMITTED rocprofv3 --kernel-trace --stats summary of the single-stream
    regime (profiles/rNN/single_stream_kernel_stats.csv: the regime the roofline block times with HIP events), all instantiations of the
    family pooled by call count -- so that `frac` can be re-derived from profiles/ alone, next to the live HIP-event mean."""
    import csv
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "single_stream_kernel_stats.csv")))
    if not files:
        return None
    try:
        calls = total = 0.0
        for row in csv.DictReader(open(files[-1])):
            if family in row["Name"]:
                calls += float(row["Calls"])
                total += float(row["TotalDurationNs"])
        if not calls:
            return None
        return {"source": os.path.relpath(files[-1], ROOT), "mean_us": round(total / calls / 1e3, 2), "calls": int(calls)}
    except Exception:
        return None


def cpu_threads_for_baseline(sd, img, O):
    """torch-CPU convolutions do not scale to every core of a large host: time the backbone once per
    candidate thread count and keep the fastest (reported as `cores`)."""
    total = os.cpu_count() or 1
    best, best_t = total, None
    for n in sorted({total, max(1, total // 2), max(1, total // 4), min(total, 64), min(total, 32), min(total, 16)}, reverse=True):
        torch.set_num_threads(n)
        with torch.no_grad():
            O.vgg16_features(sd, img)                       # warm-up at this thread count
            t0 = time.perf_counter()
            O.vgg16_features(sd, img)
            dt = time.perf_counter() - t0
        if best_t is None or dt < best_t:
            best, best_t = n, dt
    torch.set_num_threads(best)
    return best


def sample_rocm_smi(load_fn, device_index, seconds=1.2):
    """sclk / mclk / socket power of this GPU from `rocm-smi --json`, sampled while `load_fn()` keeps the headline load running
    (the tool takes a few hundred ms to start, so it is launched first and read after ~`seconds` of load).  None when unavailable."""
    import shutil
    import subprocess
    exe = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
    if not os.path.exists(exe):
        return None
    try:
        proc = subprocess.Popen([exe, "-d", str(device_index), "--showclocks", "--showpower", "--json"],
                                stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
        t_end = time.perf_counter() + seconds
        while time.perf_counter() < t_end or proc.poll() is None:
            load_fn()
            if time.perf_counter() > t_end + 10:
                proc.kill()
                return None
        raw = json.loads(proc.stdout.read().decode() or "{}")
        card = next(iter(raw.values())) if raw else {}
        out = {k: v for k, v in card.items() if any(x in k.lower() for x in ("sclk", "mclk", "power"))}
        return out or None
    except Exception:
        return None


def train_step_leg(backbone, dev, steps=10, warmup=3, lr=1e-6, pool=2, grad_math="f32", roi_pooling="pool"):
    """ms per FasterRCNNModel.train_step (one 600x1000 synthetic sample per step, batch 1 as the reference trains: forward, four
    losses, backward, SGD with momentum) -- SURVEY section 8 row f3.  grad_math="f32", RoIPool is the reference's step;
    grad_math="bf16" + roi_pooling="align" on ResNet-101 is BASELINE configs[4]'s single-GPU form."""
    import random
    from fasterrcnn_amd import synthetic, training
    from fasterrcnn_amd.datasets.training_sample import Box
    from fasterrcnn_amd.models import anchors, resnet
    from fasterrcnn_amd.models.faster_rcnn import FasterRCNNModel
    from fasterrcnn_amd.models.vgg16 import VGG16Backbone
    if backbone == "vgg16":
        model = FasterRCNNModel(num_classes=21, backbone=VGG16Backbone(dropout_probability=0.0), roi_pooling=roi_pooling)
        model.load_state_dict(synthetic.vgg16_state_dict(1234), strict=True)
        make_image = synthetic.image
    else:
        arch = {"resnet50": "ResNet50", "resnet101": "ResNet101", "resnet152": "ResNet152"}[backbone]
        model = FasterRCNNModel(num_classes=21, backbone=resnet.ResNetBackbone(getattr(resnet.Architecture, arch)), roi_pooling=roi_pooling)
        model.load_state_dict(synthetic.resnet_state_dict(1234, arch), strict=True)
        make_image = synthetic.image_rgb
    model = model.cuda(dev)
    model.grad_math = grad_math
    am, vm = anchors.generate_anchor_maps((3, H, W), model.backbone.compute_feature_map_shape((3, H, W)), 16)
    samples = []
    for seed in range(pool):
        boxes = [Box(c, "x", k) for c, k in synthetic.ground_truth(seed, H, W)]
        rmap, obj, bg = anchors.generate_rpn_map(am, vm, boxes)
        samples.append((make_image(seed, H, W).unsqueeze(0).to(dev), torch.from_numpy(rmap).unsqueeze(0).to(dev), obj, bg, boxes))
    opt = training.create_optimizer(model, learning_rate=lr)
    random.seed(0)
    torch.manual_seed(0)
    losses = []

    def step(i):
        img, rmap, obj, bg, boxes = samples[i % len(samples)]
        return model.train_step(opt, img, am, vm, rmap, [obj], [bg], [boxes])

    for i in range(warmup):
        step(i)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(steps):
        losses.append(step(i).total)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    return {"ms_per_step": round(1e3 * dt / steps, 3), "steps": steps, "math": model.math_mode,
            "dtype": "f32" if grad_math == "f32" else (
                "bf16 operands, f32 accumulation: every gradient GEMM%s; f32 master weights, losses and SGD" % (
                    " and the forward / data-gradient convolutions of the trainable bottlenecks (layer2-4)" if backbone != "vgg16" else
                    " (the 3x3 forward / data-gradient convolutions stay f32 Winograd layers)")),
            "roi": roi_pooling, "first_total_loss": round(float(losses[0]), 5), "last_total_loss": round(float(losses[-1]), 5)}


def winograd_chip_full_leg(layers, dev, streams=8, reps=6):
    """`layers`: [(name, (cin, cout, h, w))].  The float32 Winograd kernel with the chip FULL -- the regime of the headline number (several images in flight): every Winograd layer of one
    image launched back to back on each of `streams` HIP streams (own buffers per stream, random operands), wall time by events.
    achieved = streams x reps x sum of executed Winograd FLOP / wall.  A single stream (the `roofline` block) leaves the tail of every
    launch to an emptying chip: 640 work units on 512 resident-block slots (conv4_x) or 160 on 256 CUs (conv5_x)."""
    from fasterrcnn_amd import _native as nv
    lib = nv.lib()
    sts = [torch.cuda.Stream(device=dev) for _ in range(streams)]
    bufs = []
    for _ in range(streams):
        per = []
        for name, (ci, co, h, w) in layers:
            pool = name in _POOLED
            x = torch.randn((h, w, ci), device=dev)
            wt = torch.randn((co, ci, 3, 3), device=dev) * 0.02
            u = torch.empty((16 * co * ci,), device=dev)
            nv.check(lib.frcnn_pack_conv3x3_winograd_fused(nv.ptr(wt), None, nv.ptr(u), co, ci, nv.stream_ptr()), "pack")
            b = torch.zeros((co,), device=dev)
            y = torch.empty(((h // 2, w // 2, co) if pool else (h, w, co)), device=dev)
            per.append((x, u, b, y, h, w, ci, co, nv.RELU | (nv.POOL2 if pool else 0)))
        bufs.append(per)
    torch.cuda.synchronize(dev)

    def burst(n):
        for st, per in zip(sts, bufs):
            sp = st.cuda_stream
            for _ in range(n):
                for (x, u, b, y, h, w, ci, co, fl) in per:
                    nv.check(lib.frcnn_conv3x3_nhwc_winograd_fused(nv.ptr(x), nv.ptr(u), nv.ptr(b), nv.ptr(y), h, w, ci, co, fl, sp), "wino")
    t_end = time.perf_counter() + 1.0                     # clock ramp
    while time.perf_counter() < t_end:
        burst(1)
        torch.cuda.synchronize(dev)
    times = []
    for _ in range(3):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        burst(reps)
        torch.cuda.synchronize(dev)
        times.append(time.perf_counter() - t0)
    dt = sorted(times)[1]
    flops = streams * reps * sum(winograd_gemm_flops(*l) for _, l in layers)
    ach = flops / dt / 1e12
    return {"regime": "%d streams x %d repetitions of the %d Winograd layers of one image in flight (chip full), wall clock, median of 3"
                      % (streams, reps, len(layers)),
            "achieved": round(ach, 2), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / PEAK_F32_MFMA_TFLOPS, 4),
            "ms_per_image_equivalent": round(1e3 * dt / (streams * reps), 4)}


def resnet_conv_table(model, h=H, w=W, n_rois=300):
    """Every convolution of one ResNet image in execution order: (stage, name, kernel family, pipe, executed FLOP, algorithmic FLOP),
    mirroring the dispatch of csrc/api.hip's run_bottleneck for the model's current modes."""
    from fasterrcnn_amd.models import resnet as R
    fe = model._stage1_feature_extractor
    l4 = model._stage3_detector_network._pool_to_feature_vector
    wino = model.math_mode == "f32_winograd"
    rows = []
    hh, ww = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    rows.append(("backbone", "stem 7x7/s2", "conv7x7_s2_c3_kernel", "valu", 0.0, 2.0 * 147 * 64 * hh * ww))
    hh, ww = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1

    def block(stage, tag, blk, n, hh, ww, x6, single, x3=False, g3=False):
        cin, width, cout, st = blk.conv1.in_channels, blk.conv1.out_channels, blk.conv3.out_channels, blk.stride
        ho, wo = (hh - 1) // st + 1, (ww - 1) // st + 1
        if g3:      # every convolution of the block on conv_gather_x3_kernel: two fp16 terms per operand under one scale per tensor, three MFMAs per product
            convs = [(".conv1", cin, width, 1, n * hh * ww), (".conv2", width, width, 9, n * ho * wo)]
            if blk.downsample is not None:
                convs.append((".downsample", cin, cout, 1, n * ho * wo))
            convs.append((".conv3", width, cout, 1, n * ho * wo))
            for name, ci, co, taps, px in convs:
                alg = 2.0 * taps * ci * co * px
                rows.append((stage, tag + name, "conv_gather_x3_kernel", "f16", 3.0 * alg, alg))
            return ho, wo
        gk, gp, gf = ("gemm_x3t_kernel", "f16", 3.0) if x3 else ("gemm_x6t_kernel", "bf16", 6.0)     # f32x3: three fp16 MFMAs per product

        def one(name, ci, co, px, ok):
            alg = 2.0 * ci * co * px
            if x6 and wino and ok:
                rows.append((stage, tag + name, gk, gp, gf * alg, alg))
            else:
                rows.append((stage, tag + name, "conv_gather_mfma_kernel", "f32", alg, alg))
        one(".conv1", cin, width, n * hh * ww, R.x6_conv1x1_ok(cin, width))
        alg = 2.0 * 9 * width * width * n * ho * wo
        if x6 and wino and not single and width >= 256:
            if st == 1:
                rows.append((stage, tag + ".conv2", gk + " (split-operand Winograd layer)", gp,
                             gf * 2 * 16 * n * ((hh + 1) // 2) * ((ww + 1) // 2) * width * width, alg))
            else:
                rows.append((stage, tag + ".conv2", gk + " (im2col)", gp, gf * alg, alg))
        elif wino and st == 1 and single and width % 64 == 0:
            rows.append((stage, tag + ".conv2", "wino_fused_kernel", "f32", 2.0 * 16 * ((hh + 1) // 2) * ((ww + 1) // 2) * width * width, alg))
        elif wino and st == 1 and width >= 256 and width % 128 == 0:
            rows.append((stage, tag + ".conv2", "linear_mfma_kernel (three-launch Winograd)", "f32",
                         2.0 * 16 * n * ((hh + 1) // 2) * ((ww + 1) // 2) * width * width, alg))
        else:
            rows.append((stage, tag + ".conv2", "conv_gather_mfma_kernel", "f32", alg, alg))
        if blk.downsample is not None:
            one(".downsample", cin, cout, n * ho * wo, R.x6_conv1x1_ok(cin, cout))
        one(".conv3", width, cout, n * ho * wo, R.x6_conv1x1_ok(width, cout))
        return ho, wo

    seq = fe._feature_extractor
    for li, layer in ((1, seq[4]), (2, seq[5]), (3, seq[6])):
        for bi, blk in enumerate(layer):
            hh, ww = block("backbone", "layer%d.%d" % (li, bi), blk, 1, hh, ww, fe.x6_conv1x1, True, getattr(fe, "x3", False), getattr(fe, "g3", False))
    c = 1024
    alg = 2.0 * 9 * c * c * hh * ww
    if wino and "rpn_trunk" in model.winograd_x6_layers:
        t3 = "rpn_trunk" in getattr(model, "winograd_x3_layers", ())
        rows.append(("rpn", "rpn_trunk", ("gemm_x3t_kernel" if t3 else "gemm_x6t_kernel") + " (split-operand Winograd layer)", "f16" if t3 else "bf16",
                     (3.0 if t3 else 6.0) * 2 * 16 * ((hh + 1) // 2) * ((ww + 1) // 2) * c * c, alg))
    elif wino:
        rows.append(("rpn", "rpn_trunk", "wino_fused_kernel", "f32", 2.0 * 16 * ((hh + 1) // 2) * ((ww + 1) // 2) * c * c, alg))
    else:
        rows.append(("rpn", "rpn_trunk", "conv3x3_mfma_kernel", "f32", alg, alg))
    rows.append(("rpn", "rpn_heads_1x1", "linear_mfma_kernel", "f32", 2.0 * c * 45 * hh * ww, 2.0 * c * 45 * hh * ww))
    h4, w4 = 7, 7
    for bi, blk in enumerate(l4._layer4):
        h4, w4 = block("head", "layer4.%d" % bi, blk, n_rois, h4, w4, l4.x6_conv1x1, False, getattr(l4, "x3", False), getattr(l4, "g3", False))
    rows.append(("head", "detector_heads", "linear_mfma_kernel", "f32", n_rois * 2.0 * 2048 * 101, n_rois * 2.0 * 2048 * 101))
    return rows


def resnet_backbone_algorithmic_bytes(model, h=H, w=W):
    """Bytes the bottleneck convolutions of layer1..3 must move per image if every tensor crossed HBM exactly once per convolution:
    4 B x (input pixels x cin + output pixels x cout (+ the residual read) + the weights) -- DESIGN.md section 2's per-unit figure for
    conv_gather_x3_kernel -- and the number of those convolutions."""
    seq = model._stage1_feature_extractor._feature_extractor
    hh, ww = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    hh, ww = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
    total, n = 0.0, 0
    for layer in (seq[4], seq[5], seq[6]):
        for blk in layer:
            cin, width, cout, st = blk.conv1.in_channels, blk.conv1.out_channels, blk.conv3.out_channels, blk.stride
            ho, wo = (hh - 1) // st + 1, (ww - 1) // st + 1
            convs = [(hh * ww, cin, hh * ww, width, 1, False), (hh * ww, width, ho * wo, width, 9, False), (ho * wo, width, ho * wo, cout, 1, True)]
            if blk.downsample is not None:
                convs.append((hh * ww, cin, ho * wo, cout, 1, False))
            for pin, ci, pout, co, taps, res in convs:
                total += 4.0 * (pin * ci + pout * co * (2 if res else 1) + taps * ci * co)
                n += 1
            hh, ww = ho, wo
    return total, n


def resnet_roofline_leg(model, image, dev, images=6):
    """Per-kernel-class HIP-event times of ONE ResNet image at a time (slot 0) against the FLOP each class executes:
    BASELINE configs[2]'s roofline evidence.  Classes (csrc/api.hip): conv3x3_mfma = the backbone's conv_gather_mfma_kernel launches
    (exact-f32 pipe), winograd_gemm = wino_fused_kernel (backbone 3x3 + RPN trunk, exact-f32 pipe), linear_mfma = the head's float32
    launches (layer4's gather / three-launch Winograd convolutions + the RPN / detector heads), x6_gemm = gemm_x6t_kernel (bf16 pipe)."""
    for _ in range(2):
        model.predict(image, score_threshold=0.05)
    ctx = model.context(0)
    ctx.timing_enable(True)
    per = []
    for _ in range(images):
        model.predict(image, score_threshold=0.05)
        torch.cuda.synchronize(dev)
        per.append(ctx.timing_read(reset=True))
    ctx.timing_enable(False)
    med = {k: sorted(t[k][0] for t in per)[len(per) // 2] for k in per[0]}
    launches = {k: per[0][k][1] for k in per[0]}
    table = resnet_conv_table(model)
    by = {"conv3x3_mfma": 0.0, "winograd_gemm": 0.0, "linear_mfma": 0.0, "winograd_x6_gemm": 0.0}
    alg_backbone = 0.0
    g3_backbone = bool(getattr(model._stage1_feature_extractor, "g3", False))
    for stage, name, kern, pipe, ex, alg in table:
        if kern.startswith("gemm_x6t") or kern.startswith("gemm_x3t"):
            by["winograd_x6_gemm"] += ex
        elif kern.startswith("wino_fused"):
            by["winograd_gemm"] += ex
        elif stage == "backbone" and kern.startswith("conv_gather"):       # timing class 0: every launch of run_bottleneck's backbone blocks
            by["conv3x3_mfma"] += ex
            alg_backbone += alg
        elif kern.startswith("conv_gather_x3"):                              # layer4 with bottleneck_g3 = "all": timed with the head's launches
            by["linear_mfma"] += alg
        elif pipe == "f32":
            by["linear_mfma"] += ex
    out = {"regime": "HIP events around every launch, one image at a time on one stream, median image of %d" % images,
           "ms_per_image_by_class": {k: round(v, 4) for k, v in med.items()}, "launches_by_class": launches, "classes": {}}
    for cls, peak, unit in (("conv3x3_mfma", PEAK_BF16_MFMA_TFLOPS if g3_backbone else PEAK_F32_MFMA_TFLOPS, "fp16 (f32x3)" if g3_backbone else "f32"),
                            ("winograd_gemm", PEAK_F32_MFMA_TFLOPS, "f32"),
                            ("linear_mfma", PEAK_F32_MFMA_TFLOPS, "f32"), ("winograd_x6_gemm", PEAK_BF16_MFMA_TFLOPS, "bf16 / fp16")):
        if med.get(cls, 0.0) > 0 and by[cls] > 0:
            ach = by[cls] / (med[cls] / 1e3) / 1e12
            out["classes"][cls] = {"pipe": unit, "executed_gflop_per_image": round(by[cls] / 1e9, 2), "ms_per_image": round(med[cls], 4),
                                   "achieved_tflops": round(ach, 2), "peak": peak, "frac": round(ach / peak, 4)}
    dom = max(out["classes"], key=lambda k: out["classes"][k]["ms_per_image"]) if out["classes"] else None
    if g3_backbone and "conv3x3_mfma" in out["classes"]:
        # what an exact-f32 kernel would have to sustain to match: the layer's algorithmic FLOP against the float32 matrix peak
        c0 = out["classes"]["conv3x3_mfma"]
        c0["f32_equivalent_tflops"] = round(alg_backbone / (med["conv3x3_mfma"] / 1e3) / 1e12, 2)
        c0["f32_equivalent_frac_of_f32_peak"] = round(c0["f32_equivalent_tflops"] / PEAK_F32_MFMA_TFLOPS, 4)
        c0["note"] = ("conv_gather_x3_kernel is bound by the L2 -> CU fetch of its operand tiles (tools/gx_clocks.py: a stage takes the time its "
                      "16-32 KB take at ~40 GB/s per CU), not by the matrix pipe")
    kernel_of = {"conv3x3_mfma": ("conv_gather_x3_kernel (every backbone bottleneck convolution, f32x3 under one scale per tensor)" if g3_backbone else
                                  "conv_gather_mfma_kernel (backbone 1x1 / strided convolutions, exact-f32 pipe)"),
                 "winograd_gemm": "wino_fused_kernel (backbone 3x3 + RPN trunk)", "linear_mfma": "the head's float32 launches",
                 "winograd_x6_gemm": "gemm_x3t_kernel / gemm_x6t_kernel (layer4's convolutions and the RPN trunk as split-operand GEMMs)"}
    if dom and g3_backbone and dom == "conv3x3_mfma":
        # the f32x3 gather kernel: of the two rooflines the HBM one binds (its algorithmic bytes take longer at 8 TB/s than its matrix
        # instructions at the fp16 peak); what actually limits it is the L2 -> CU fetch in between (the class note)
        abytes, nconv = resnet_backbone_algorithmic_bytes(model)
        gbs = abytes / (med[dom] / 1e3) / 1e9
        out.update({"kernel": kernel_of[dom], "bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                    "frac": round(gbs / PEAK_HBM_GBS, 4), "traffic": measured_traffic("conv_gather_x3_kernel"),
                    "algorithmic_bytes_per_launch": abytes / nconv, "launches_per_image": nconv,
                    "mfma_frac": out["classes"][dom]["frac"],
                    "note": "achieved = algorithmic bytes of the %d bottleneck convolutions (each tensor once per convolution) / the class's HIP-event "
                            "time; traffic = measured HBM bytes per launch (profiles/, FETCH_SIZE x 2 + WRITE_SIZE)" % nconv})
    elif dom:
        out.update({"kernel": kernel_of[dom], "bound": "mfma", "achieved": out["classes"][dom]["achieved_tflops"], "peak": out["classes"][dom]["peak"],
                    "unit": "TFLOP/s", "frac": out["classes"][dom]["frac"], "traffic": measured_traffic("conv_gather_mfma_kernel")})
    return out


def winograd_layer_fracs(dev, reps=12):
    """Per-layer durations of the dominant kernel (wino_x3d_kernel) on the shapes of the 13 one-launch layers, each launched back to back on the
    current stream with its input's channel maxima given (as the forward chains them), HIP events around `reps` launches: the per-layer
    fractions the averaged `roofline.frac` hides (0.13 on conv5_x's 80 blocks ... 0.24 on conv3_3)."""
    from fasterrcnn_amd import _native as nv
    lib, sp = nv.lib(), nv.stream_ptr()
    shapes = [("conv1_2", 64, 64, 600, 1000, True, 1), ("conv2_1", 64, 128, 300, 500, False, 1), ("conv2_2", 128, 128, 300, 500, True, 1),
              ("conv3_1", 128, 256, 150, 250, False, 1), ("conv3_2", 256, 256, 150, 250, False, 1), ("conv3_3", 256, 256, 150, 250, True, 1),
              ("conv4_1", 256, 512, 75, 125, False, 1), ("conv4_2", 512, 512, 75, 125, False, 1), ("conv4_3", 512, 512, 75, 125, True, 1),
              ("conv5_x + rpn_trunk", 512, 512, 37, 62, False, 4)]
    rows = []
    for name, cin, cout, h, w, pool, count in shapes:
        x = torch.randn((h, w, cin), device=dev).clamp(min=0)
        wt = torch.randn((cout, cin, 3, 3), device=dev) * 0.02
        b = torch.zeros((cout,), device=dev)
        bank = torch.empty((16, cout, cin), device=dev)
        u = torch.empty((int(lib.frcnn_conv3x3_winograd_x3_pack_bytes(cout, cin)),), dtype=torch.int8, device=dev)
        nv.check(lib.frcnn_pack_conv3x3_winograd(nv.ptr(wt), None, nv.ptr(bank), cout, cin, sp), "pack")
        nv.check(lib.frcnn_pack_conv3x3_winograd_x3(nv.ptr(bank), nv.ptr(u), cout, cin, sp), "pack_x3")
        oh, ow = (h // 2, w // 2) if pool else (h, w)
        y = torch.empty((oh, ow, cout), device=dev)
        wsb = int(lib.frcnn_conv3x3_winograd_x3_fused_workspace_bytes(1, h, w))
        ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        cm = torch.empty((h, w), device=dev)
        nv.check(lib.frcnn_pixel_absmax(nv.ptr(x), nv.ptr(cm), h * w, cin, sp), "absmax")
        flags = nv.RELU | (nv.POOL2 if pool else 0)

        def call():
            nv.check(lib.frcnn_conv3x3_nhwc_winograd_x3_chain(nv.ptr(x), nv.ptr(u), nv.ptr(b), nv.ptr(y), 1, h, w, cin, cout, flags, 1, nv.ptr(ws), wsb,
                                                              nv.ptr(cm), None, sp), "x3_chain")
        for _ in range(3):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize(dev)
        us = e0.elapsed_time(e1) * 1e3 / reps
        fl = 3.0 * winograd_gemm_flops(cin, cout, h, w)
        rows.append({"layer": name, "launches_per_image": count, "cin": cin, "cout": cout, "h": h, "w": w, "us": round(us, 1),
                     "executed_gflop": round(fl / 1e9, 2), "frac": round(fl / (us * 1e-6) / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4)})
    return rows


def parity_leg(model, slot, make_image, dev):
    """north_star's bar measured in THIS process on the arithmetic table the headline runs (in-flight slot `slot`), against committed fixtures only
    (tests/golden/: arrays written from the imported reference and the float64 truth by oracle/make_golden.py / make_holdout.py; nothing
    under oracle/ is imported here):
      golden 600x1000 image: rows of the reference reproduced AT THEIR INDEX within 1e-3 px (forward: proposals; predict: detections per class
          in the reference's order), and the worst row;
      held-out set (the fixtures that share the bench model's weights seed): the same fractions, and K = our distance from the float64 truth
          relative to the reference's own (median / p95 over rows, median over images) -- the admission criterion of DESIGN.md section 4."""
    import glob
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden")
    gate = 1e-3

    def run(g):
        img = make_image(int(g["seed"]), int(g["height"]), int(g["width"])).unsqueeze(0).to(dev)
        with torch.no_grad():
            props, _, _ = model._enqueue(img, None, None, None, slot).result()
        det = model.predict_async(img, float(g["score_threshold"]), slot).result()
        return props.cpu().numpy().astype(np.float64), det

    def rows_at_index(ours, ref):
        n = max(len(ours), len(ref))
        err = np.full(n, np.inf)
        m = min(len(ours), len(ref))
        if m:
            err[:m] = np.abs(ours[:m, :4] - np.asarray(ref, dtype=np.float64)[:m, :4]).max(axis=1)
        return err

    def det_rows(det, ref):          # ref rows: [class, y1, x1, y2, x2, score]
        ok, worst = 0, 0.0
        for c in np.unique(ref[:, 0]) if len(ref) else []:
            r = ref[ref[:, 0] == c][:, 1:]
            e = rows_at_index(np.asarray(det[int(c)], dtype=np.float64), r)[: len(r)]
            ok += int((e <= gate).sum())
            fin = e[np.isfinite(e)]
            worst = max(worst, float(fin.max()) if fin.size else 0.0)
        return ok, worst

    out = {"gate_px": gate, "slot": slot, "source": "tests/golden fixtures (reference rows + float64 truth), same process, the headline's arithmetic table"}
    g = np.load(os.path.join(root, "vgg16_600x1000_s0.npz"))
    ours, det = run(g)
    e = rows_at_index(ours, g["proposals"])
    d_ok, d_worst = det_rows(det, g["detections"])
    out["golden_600x1000"] = {"forward_rows_within_gate": int((e <= gate).sum()), "forward_rows": int(len(e)), "forward_worst_row_px": float(e[np.isfinite(e)].max()),
                              "predict_rows_within_gate": d_ok, "predict_rows": int(len(g["detections"])), "predict_worst_row_px": d_worst}
    files = [f for f in sorted(glob.glob(os.path.join(root, "holdout", "vgg16_*_w1234.npz")))]
    p_ok = p_n = dd_ok = dd_n = 0
    med, p95, rmed, rp95 = [], [], [], []
    for f in files:
        g = np.load(f)
        ours, det = run(g)
        e = rows_at_index(ours, g["ref_proposals"])
        p_ok += int((e <= gate).sum()); p_n += int(len(e))
        k, _ = det_rows(det, g["ref_detections"])
        dd_ok += k; dd_n += int(len(g["ref_detections"]))
        # distance of every row of ours from the NEAREST float64 candidate box (a proposal is the decode of one anchor)
        tb = g["truth_cand_boxes"]
        err = np.array([np.abs(tb - row[None, :]).max(axis=1).min() for row in ours[:, :4]])
        fin = err[np.isfinite(err) & (err <= 0.5)]
        ref = g["ref_prop_err"]
        rfin = ref[np.isfinite(ref) & (ref <= 0.5)]
        med.append(float(np.median(fin))); p95.append(float(np.percentile(fin, 95)))
        rmed.append(float(np.median(rfin))); rp95.append(float(np.percentile(rfin, 95)))
    if files:
        out["held_out"] = {"images": len(files), "proposal_rows_within_gate": p_ok, "proposal_rows": p_n, "detection_rows_within_gate": dd_ok, "detection_rows": dd_n,
                           "proposals_vs_float64_truth_px": {"median": float(np.median(med)), "p95": float(np.median(p95))},
                           "reference_vs_float64_truth_px": {"median": float(np.median(rmed)), "p95": float(np.median(rp95))},
                           "K_median": round(float(np.median(med)) / float(np.median(rmed)), 3), "K_p95": round(float(np.median(p95)) / float(np.median(rp95)), 3)}
    return out


def planted_ground_truth(seed, det, num_classes=21):
    """Synthetic GT for image `seed`: seeded random boxes plus up to 3 of the image's own top
    detections jittered by a few pixels (so mAP@0.5 is neither 0 nor 1)."""
    from fasterrcnn_amd import synthetic
    from fasterrcnn_amd.datasets.training_sample import Box
    rng = np.random.RandomState(104729 * int(seed) + 1)
    boxes = [Box(c, str(c), k) for c, k in synthetic.ground_truth(seed, H, W, num_classes)]
    rows = [(c, r) for c, v in det.items() for r in v[:2]]
    rows.sort(key=lambda cr: -cr[1][4])
    for c, r in rows[:3]:
        boxes.append(Box(int(c), str(c), (r[:4] + rng.randn(4) * 4.0).astype(np.float32)))
    return boxes


def pack_detections(det):
    """predict()'s dict {class: (n, 5) rows of (y1, x1, y2, x2, score)} as the two float64 arrays --dump-outputs writes: (N, 6) rows of
    (class, y1, x1, y2, x2, score) in class order -- a class with no detection contributes no row -- and the row count of each class, in
    the same order, which rebuilds the dict from the rows."""
    det = sorted(det.items())
    rows = [np.concatenate([np.full((len(r), 1), c, dtype=np.float64), np.asarray(r, dtype=np.float64).reshape(-1, 5)], axis=1) for c, r in det]
    return (np.concatenate(rows, axis=0) if rows else np.zeros((0, 6))), np.array([len(r) for _, r in det], dtype=np.float64)


def hw_queues(environ=None):
    """GPU_MAX_HW_QUEUES as the environment sets it (int), or None when unset: the HIP runtime then uses its own default."""
    v = (os.environ if environ is None else environ).get("GPU_MAX_HW_QUEUES")
    return int(v) if v else None


def launcher_command(gpus, argv, environ=None):
    """(command, environment) that re-runs this file as `gpus` ranks of ONE node under torch.distributed.run -- exactly the form the
    driver uses for N > 1 (docstring above): rendezvous on 127.0.0.1 (the container hostname may not resolve), a free port, the
    caller's flags passed through.  The environment adds what a multi-process GPU job needs on this stack: dmabuf IPC for RCCL
    (HSA_ENABLE_IPC_MODE_LEGACY=0); the HIP hardware-queue count is the caller's environment's."""
    import socket
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(int(gpus)),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ if environ is None else environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return cmd, env


def rank_environment(environ=None):
    """(rank, local_rank, world) as torch.distributed.run exports them; a plain `python bench.py` is rank 0 of 1.  LOCAL_RANK is the
    HIP device index of the rank (one process per GPU)."""
    e = os.environ if environ is None else environ
    return int(e.get("RANK", "0")), int(e.get("LOCAL_RANK", "0")), int(e.get("WORLD_SIZE", "1"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--inflight", type=int, default=4,
                    help="images in flight per GPU (separate HIP streams).  Every VGG-16 layer fills the chip from one image, so the images in "
                         "flight only have to cover each other's serial proposal / detection tails; round 6, same box: 3 / 4 / 5 in flight = "
                         "922-925 / 933-936 / 827-839 images/sec in bursts of 20 (7 + 7 + 6 against 5 + 5 + 5 + 5 images per slot) and "
                         "959 / 972 / 856 in steady state (profiles/r06/exp_inflight_driver.txt)")
    ap.add_argument("--hip-graphs", action="store_true",
                    help="replay one captured hipGraph per in-flight slot instead of ~39 eager launches per image (FasterRCNNModel.use_hip_graphs)")
    ap.add_argument("--pool", type=int, default=8, help="distinct synthetic images resident per GPU")
    ap.add_argument("--map-images", type=int, default=8, help="labelled images per rank for the mAP@0.5 leg")
    ap.add_argument("--cpu-images", type=int, default=12, help="images timed on the host CPU (rank 0, N=1 only): ~12 s of CPU work")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--roofline-images", type=int, default=10)
    ap.add_argument("--math", type=str, default=None, choices=["f32", "f32_winograd"],
                    help="3x3 conv arithmetic: f32_winograd (default: exact f32 MFMA, every 3x3 layer from conv1_2 on as a one-launch Winograd "
                         "F(2x2,3x3) layer in float32) or f32 (every layer on the direct exact-f32 kernel)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the informational legs in the other math modes")
    ap.add_argument("--ramp-seconds", type=float, default=2.0,
                    help="untimed pre-roll before the warm-up steps: the GPU takes ~1-2 s of load to leave its idle power state "
                         "(sclk 157 MHz -> 2.4 GHz), far longer than a 20-step warm-up")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise the RCCL process group and run every barrier / all-reduce / all-gather also with ONE rank "
                         "(so the multi-GPU code path can be exercised on a one-GPU box)")
    ap.add_argument("--min-timed-seconds", type=float, default=0.0,
                    help="the timed burst of --steps steps is repeated until this much has been timed; the MEDIAN burst is reported "
                         "(default 0: ONE burst, i.e. exactly --steps timed steps)")
    ap.add_argument("--no-extra-legs", action="store_true", help="skip the single-stream / ResNet-50 / train-step legs")
    ap.add_argument("--backbone", type=str, default="vgg16", choices=["vgg16", "resnet50", "resnet101", "resnet152"],
                    help="vgg16 is the BASELINE.json metric; the ResNets are informational (configs[2])")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step returned (predict()'s per-class (n, 5) float64 detections) "
                         "as DIR/detections.npy, (N, 6) rows of (class, y1, x1, y2, x2, score) in class order, and "
                         "DIR/detections_per_class.npy, the row count of each class 1..20; rank 0 only")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run every other leg: the other arithmetic tables, host-fed, single-stream, ResNet-50 and "
                         "train-step legs, per-rank burst, clocks under load, parity, host CPU per image, mAP@0.5, roofline, CPU baseline "
                         "(the --no-* options and --map-images / --roofline-images / --cpu-images shape them); off by default")
    args = ap.parse_args()

    rank, local_rank, world = rank_environment()
    if world == 1 and args.gpus > 1:
        # started without a launcher: re-run under torch.distributed.run, one rank per GPU (the form the docstring shows)
        import subprocess
        cmd, env = launcher_command(args.gpus, sys.argv[1:])
        sys.exit(subprocess.call(cmd, env=env))
    use_dist = world > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if "MASTER_ADDR" not in os.environ:          # --force-dist without a launcher
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("MASTER_PORT", "29531"), RANK="0", WORLD_SIZE="1")
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
    n_gpus = world
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    from fasterrcnn_amd import _native, synthetic
    from fasterrcnn_amd.evaluate import ImageRecords, merged_calculator
    from fasterrcnn_amd.models.faster_rcnn import FasterRCNNModel
    from fasterrcnn_amd.models.vgg16 import VGG16Backbone
    _native.require_gpu()

    is_resnet = args.backbone != "vgg16"
    if is_resnet:
        from fasterrcnn_amd.models import resnet
        arch = {"resnet50": "ResNet50", "resnet101": "ResNet101", "resnet152": "ResNet152"}[args.backbone]
        sd = synthetic.resnet_state_dict(1234, arch)
        model = FasterRCNNModel(num_classes=21, backbone=resnet.ResNetBackbone(getattr(resnet.Architecture, arch)))
    else:
        sd = synthetic.vgg16_state_dict(1234)
        model = FasterRCNNModel(num_classes=21, backbone=VGG16Backbone(dropout_probability=0.0))
    model.load_state_dict(sd, strict=True)
    model = model.cuda(dev).eval()
    if args.math is None:
        args.math = model.math_mode                 # the model's default: f32_winograd (VGG-16) / f32 (ResNet)
    model.math_mode = args.math
    if args.hip_graphs:
        model.use_hip_graphs = True
    make_image = synthetic.image_rgb if is_resnet else synthetic.image

    # synthetic image pool, resident in HBM before timing; per-image seed = global index
    seeds = [rank * args.pool + i for i in range(args.pool)]
    pool = [make_image(s).unsqueeze(0).to(dev) for s in seeds]
    nslots = max(1, args.inflight)

    def run(n_steps):
        pending = []
        for i in range(n_steps):
            if len(pending) == nslots:
                pending.pop(0).result()
            # one image at a time = slot 0 (the latency configuration of predict()); otherwise the in-flight slots 1..n
            pending.append(model.predict_async(pool[i % len(pool)], 0.05, slot=0 if nslots == 1 else 1 + (i % nslots)))
        last = None
        while pending:
            last = pending.pop(0).result()
        return last

    last_step = {}

    def timed_burst(fn, n_steps):
        """EXACTLY n_steps steps bracketed by barrier + synchronize on both sides; MAX over ranks."""
        torch.cuda.synchronize(dev)
        if use_dist:
            dist.barrier()
        ts = time.perf_counter()
        last_step["out"] = fn(n_steps)
        torch.cuda.synchronize(dev)
        if use_dist:
            dist.barrier()
        dt = time.perf_counter() - ts
        if use_dist:
            tt = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt.item())
        return dt

    def timed_median(fn, n_steps, min_seconds):
        """Repeats the K-step burst until `min_seconds` have been timed (at least once, at most 64 times; every rank takes
        the same decision because the burst time is already the max over ranks) and returns (median burst, all bursts)."""
        bursts, total = [], 0.0
        while not bursts or (total < min_seconds and len(bursts) < 64):
            bursts.append(timed_burst(fn, n_steps))
            total += bursts[-1]
        srt = sorted(bursts)
        return srt[(len(srt) - 1) // 2], bursts

    t_ramp = time.perf_counter() + max(args.ramp_seconds, 0.0)
    while time.perf_counter() < t_ramp:
        run(nslots)
    run(max(args.warmup, nslots))
    elapsed, bursts = timed_median(run, args.steps, args.min_timed_seconds)
    value = n_gpus * args.steps / elapsed
    if args.dump_outputs and rank == 0:
        # the last timed step: image pool[(steps - 1) % pool], seeded, so the same flags give the same input on every run
        os.makedirs(args.dump_outputs, exist_ok=True)
        rows, counts = pack_detections(last_step["out"])
        np.save(os.path.join(args.dump_outputs, "detections.npy"), rows)
        np.save(os.path.join(args.dump_outputs, "detections_per_class.npy"), counts)
    # ---- --full only from here on: every leg below is informational, outside the timed region, and not the headline value ----------
    # per-rank view of the same timed region (each rank's own wall time of its median burst is not kept: the burst time is already the
    # max over ranks; what differs per rank is its LOCAL burst, measured here without the barrier), gathered for the JSON line
    per_rank = None
    if args.full:
        torch.cuda.synchronize(dev)
        t_loc = time.perf_counter()
        run(args.steps)
        torch.cuda.synchronize(dev)
        local_ips = args.steps / (time.perf_counter() - t_loc)
        per_rank = [round(local_ips, 3)]
        if use_dist:
            tt = torch.zeros(world, dtype=torch.float64, device=dev)
            tt[rank] = local_ips
            dist.all_reduce(tt, op=dist.ReduceOp.SUM)
            per_rank = [round(float(v), 3) for v in tt.tolist()]

    # clocks / power under the headline load (rocm-smi sampled in the middle of one more, untimed, second of the same load)
    smi = None
    if rank == 0 and args.full:
        smi = sample_rocm_smi(lambda: run(nslots), local_rank)

    # ---- informational: the same workload in the other math modes (not the headline value) -----------
    secondary = {}
    if args.full and not is_resnet and not args.no_secondary:
        for mode in ("f32", "f32_winograd"):
            if mode == args.math:
                continue
            model.math_mode = mode
            run(max(args.warmup, nslots))
            dt, _ = timed_median(run, args.steps, min(args.min_timed_seconds, 0.5))
            secondary[mode] = round(n_gpus * args.steps / dt, 3)
        model.math_mode = args.math
    fc_math = model.fc_math_mode
    x6 = tuple(getattr(model, "winograd_x6_layers", ())) if args.math == "f32_winograd" else ()
    x3 = tuple(getattr(model, "winograd_x3_layers", ())) if args.math == "f32_winograd" else ()
    x3f = tuple(n_ for n_ in getattr(model, "winograd_x3f_layers", ()) if n_ not in x6) if (args.math == "f32_winograd" and not is_resnet) else ()
    fc_f32_value = None
    if args.full and not is_resnet and not args.no_secondary and fc_math != "f32":
        # the same workload with fc1 / fc2 on the exact-f32 pipe too: every GEMM of the image on v_mfma_f32_*_f32
        model.fc_math_mode = "f32"
        run(max(args.warmup, nslots))
        dt, _ = timed_median(run, args.steps, min(args.min_timed_seconds, 0.5))
        fc_f32_value = round(n_gpus * args.steps / dt, 3)
        model.fc_math_mode = fc_math
        run(nslots)

    wino_f32_value = None
    if args.full and not is_resnet and not args.no_secondary and (x6 or x3f):
        # the same workload with EVERY 3x3 layer on the exact-f32 pipe (rounds 1-2's default table: no x6 Winograd layer)
        model.winograd_x6_layers = ()
        model.winograd_x3f_layers = ()
        run(max(args.warmup, nslots))
        dt, _ = timed_median(run, args.steps, min(args.min_timed_seconds, 0.5))
        wino_f32_value = round(n_gpus * args.steps / dt, 3)
        model.winograd_x6_layers = x6
        model.winograd_x3_layers = x3
        model.winograd_x3f_layers = x3f
        run(nslots)

    strict_f32_value = None
    if args.full and not is_resnet and not args.no_secondary and (x6 or x3f or fc_math != "f32"):
        # STRICT float32: every GEMM of the image on the exact-f32 matrix instructions (no split-operand layer anywhere)
        model.winograd_x6_layers = ()
        model.winograd_x3f_layers = ()
        model.fc_math_mode = "f32"
        run(max(args.warmup, nslots))
        dt, _ = timed_median(run, args.steps, min(args.min_timed_seconds, 0.5))
        strict_f32_value = round(n_gpus * args.steps / dt, 3)
        model.winograd_x6_layers = x6
        model.winograd_x3_layers = x3
        model.winograd_x3f_layers = x3f
        model.fc_math_mode = fc_math
        run(nslots)

    # ---- end-to-end leg: the host -> device step of the reference's loop INSIDE the timed region ----------------
    # __main__.py:78-86 uploads every image inside the loop (`t.from_numpy(image).unsqueeze(0).cuda()`), predict_one (:237-240) also
    # resizes / normalises it first (datasets/image.py:59-101).  Here: decoded uint8 frames in pinned host memory -> async H2D on the
    # slot's feeder stream -> frcnn_preprocess (PIL-exact resize 375x625 -> 600x1000 + normalisation) -> predict_async; and the
    # reference's literal form, the preprocessed float32 tensor uploaded as is (7.2 MB per image).
    h2d = {}
    if args.full and not is_resnet and not args.no_secondary:
        from fasterrcnn_amd.evaluate import HostFeeder
        feeder = HostFeeder(model, lookahead=2 * nslots)
        host_u8 = [synthetic.image_u8(s_).pin_memory() for s_ in seeds]
        host_f32 = [p_[0].cpu().pin_memory() for p_ in pool]

        def run_host(submit, frames):
            def fn(n_steps):
                pending = []
                for i in range(n_steps):
                    if len(pending) == nslots:
                        pending.pop(0).result()
                    pending.append(submit(frames[i % len(frames)], 0.05, 1 + (i % nslots)))
                while pending:
                    pending.pop(0).result()
            return fn

        def run_staged(n_steps):
            # frames are staged (H2D + resize + normalise on the feeder ring) `nslots` images ahead of their predict
            staged, pending = [], []
            for i in range(min(nslots, n_steps)):
                staged.append(feeder.stage(host_u8[i % len(host_u8)]))
            for i in range(n_steps):
                if len(pending) == nslots:
                    pending.pop(0).result()
                pending.append(feeder.submit_staged(staged.pop(0), 0.05, 1 + (i % nslots)))
                if i + nslots < n_steps:
                    staged.append(feeder.stage(host_u8[(i + nslots) % len(host_u8)]))
            while pending:
                pending.pop(0).result()
        for key, fn in (("h2d_preprocess_images_per_sec", run_host(feeder.submit, host_u8)),
                        ("h2d_preprocess_staged_images_per_sec", run_staged),
                        ("h2d_float32_images_per_sec", run_host(feeder.submit_preprocessed, host_f32))):
            fn(max(args.warmup, nslots))
            dt, _ = timed_median(fn, args.steps, min(args.min_timed_seconds, 0.5))
            h2d[key] = round(n_gpus * args.steps / dt, 3)
        h2d["h2d_note"] = ("the headline loop fed from PINNED HOST memory inside the timed region: h2d_preprocess = uint8 375x625 RGB frame -> async "
                           "H2D (0.7 MB) -> frcnn_preprocess (PIL-exact resize to 600x1000 + normalisation on the device) -> predict (HostFeeder.submit); "
                           "_staged = the same with the frames staged as many images ahead as there are in flight (HostFeeder.stage / submit_staged: "
                           "measured no better -- the copy + resize of one image already overlap the other images' convolutions); h2d_float32 = the "
                           "reference's literal `t.from_numpy(image).cuda()` of the preprocessed 3x600x1000 float32 tensor (7.2 MB) -> predict")
        del feeder, host_u8, host_f32
        run(nslots)

    x3_legs = {}
    if args.full and not is_resnet and not args.no_secondary and x3f:
        # conv1_2 .. conv3_3 back on the float32 one-launch Winograd kernel and the 512-channel layers on their three launches in every slot
        # (round 3's pipeline for those layers)
        inflight_x3f = model.inflight_winograd_x3f_layers
        model.winograd_x3f_layers = ()
        model.inflight_winograd_x3f_layers = ()
        run(max(args.warmup, nslots))
        dt, _ = timed_median(run, args.steps, min(args.min_timed_seconds, 0.5))
        x3_legs["no_one_launch_x3_layers_images_per_sec"] = round(n_gpus * args.steps / dt, 3)
        model.winograd_x3f_layers = x3f
        model.inflight_winograd_x3f_layers = inflight_x3f
        run(nslots)
    if args.full and not is_resnet and not args.no_secondary and x6:
        # the f32x3 arithmetic switched off (every split-operand GEMM in f32x6: the table before the f32x3 kernels existed), and round 3's
        # default table (conv5_1 kept in f32x6 because one box of one golden fixture then landed at 0.92e-3 instead of 1.04e-3 px; round 4
        # chooses the table against the float64 truth on held-out images instead: DESIGN.md section 4)
        for key, layers, fcm in (("f32x6_only_images_per_sec", (), "f32x6" if fc_math == "f32x3" else fc_math), ("round3_table_images_per_sec", tuple(n_ for n_ in x6 if n_ != "conv5_1"), fc_math)):
            model.winograd_x3_layers, model.fc_math_mode = layers, fcm
            run(max(args.warmup, nslots))
            dt, _ = timed_median(run, args.steps, min(args.min_timed_seconds, 0.5))
            x3_legs[key] = round(n_gpus * args.steps / dt, 3)
        model.winograd_x3_layers, model.fc_math_mode = x3, fc_math
        run(nslots)

    # ---- driver-timed secondary legs (rank 0 of a one-GPU run; none of them is the headline value) -------------------
    extra = {}
    if rank == 0 and args.full and n_gpus == 1 and not args.no_extra_legs and not is_resnet:
        # (1) configs[1] taken literally: ONE image on the chip at a time (slot 0 = the latency configuration of predict())
        def run_single(n_steps):
            for i in range(n_steps):
                model.predict(pool[i % len(pool)], score_threshold=0.05)
        run_single(5)
        dt, _ = timed_median(run_single, args.steps, min(args.min_timed_seconds, 0.5))
        extra["single_stream_images_per_sec"] = round(args.steps / dt, 3)
        # (2) configs[2]: ResNet-50 backbone, independent batch-1 images in flight (the reference asserts batch 1)
        from fasterrcnn_amd.models import resnet as _resnet
        m50 = FasterRCNNModel(num_classes=21, backbone=_resnet.ResNetBackbone(_resnet.Architecture.ResNet50))
        m50.load_state_dict(synthetic.resnet_state_dict(1234, "ResNet50"), strict=True)
        m50 = m50.cuda(dev).eval()
        pool50 = [synthetic.image_rgb(s_).unsqueeze(0).to(dev) for s_ in seeds[:8]]
        # images in flight: one per hardware pipe, on the process's slot streams (runtime.slot_stream: the streams VGG-16's slots used above);
        # round 6: 4 in flight 702 / 679 images/sec steady / bursts of 20, 8 in flight 693 / 670 (profiles/r06/exp_r50_inflight.txt)
        from fasterrcnn_amd.evaluate import default_inflight
        n50 = default_inflight(m50)

        def run50(n_steps):
            pend = []
            for i in range(n_steps):
                if len(pend) == n50:
                    pend.pop(0).result()
                pend.append(m50.predict_async(pool50[i % len(pool50)], 0.05, slot=1 + (i % n50)))
            while pend:
                pend.pop(0).result()
        run50(16)
        dt, _ = timed_median(run50, args.steps, min(args.min_timed_seconds, 0.5))
        extra["resnet50_images_per_sec"] = round(args.steps / dt, 3)
        extra["resnet50_config"] = ("ResNet-50 predict(), 3x600x1000, %d batch-1 images in flight, math %s, bottleneck_g3=%s (layer1..3: every bottleneck "
                                    "convolution in the f32x3 arithmetic under one scale per tensor, conv_gather_x3_kernel, weight packs split at pack time), x6_conv1x1=%s in the %s arithmetic (the "
                                    "convolutions of the per-RoI layer4 as split-operand GEMMs on the fp16 / bf16 matrix instructions), winograd_x6_layers=%s, "
                                    "winograd_x3_layers=%s; every golden proposal / detection reproduced"
                                    % (n50, m50.math_mode, m50.bottleneck_g3, m50.x6_conv1x1, m50.x6_conv1x1_arith, list(m50.winograd_x6_layers),
                                       list(m50.winograd_x3_layers)))
        d50 = dict(x6_conv1x1=m50.x6_conv1x1, x6_conv1x1_arith=m50.x6_conv1x1_arith, winograd_x6_layers=m50.winograd_x6_layers,
                   winograd_x3_layers=m50.winograd_x3_layers, bottleneck_g3=m50.bottleneck_g3)

        def set50(**kw):
            for k_, v_ in kw.items():
                setattr(m50, k_, v_)
        # the OPTION bottleneck_g3 = "all" (round 6: with the weight packs split at pack time it is the fastest table): layer4's per-RoI
        # convolutions under one scale per tensor too -- admitted by the held-out sweep (same counts and K as the default), not the default:
        # one golden detection of the batch-8 fixture moves past 1e-3 px (tests/test_resnet_gpu.py holds it to the observed counts)
        set50(bottleneck_g3="all")
        run50(16)
        dt, _ = timed_median(run50, args.steps, min(args.min_timed_seconds, 0.5))
        extra["resnet50_g3_all_images_per_sec"] = round(args.steps / dt, 3)
        set50(**d50)
        # round 3's default: the backbone on the exact-f32 gather / float32 Winograd kernels
        set50(bottleneck_g3="off")
        run50(16)
        dt, _ = timed_median(run50, args.steps, min(args.min_timed_seconds, 0.5))
        extra["resnet50_f32_backbone_images_per_sec"] = round(args.steps / dt, 3)
        # ... with every eligible 1x1 convolution of that backbone (layer2 / layer3) as a row-scaled split-operand GEMM
        set50(x6_conv1x1="all")
        run50(16)
        dt, _ = timed_median(run50, args.steps, min(args.min_timed_seconds, 0.5))
        extra["resnet50_x6_all_images_per_sec"] = round(args.steps / dt, 3)
        # the default of the first half of round 3: layer4 in f32x6, RPN trunk on the float32 one-launch Winograd kernel
        set50(x6_conv1x1="head", x6_conv1x1_arith="f32x6", winograd_x6_layers=(), winograd_x3_layers=())
        run50(16)
        dt, _ = timed_median(run50, args.steps, min(args.min_timed_seconds, 0.5))
        extra["resnet50_f32x6_head_images_per_sec"] = round(args.steps / dt, 3)
        set50(x6_conv1x1="off")
        run50(16)
        dt, _ = timed_median(run50, args.steps, min(args.min_timed_seconds, 0.5))
        extra["resnet50_all_f32_pipe_images_per_sec"] = round(args.steps / dt, 3)
        set50(**d50)
        # configs[2] as a TRUE batch: 8 images through one pass of the feature extractor (frcnn_resnet_backbone: every bottleneck launch
        # covers the 8 maps), RPN + head per image on 8 streams behind it; two batches in flight
        try:
            batch50 = torch.cat(pool50, dim=0)

            def run50b(n_steps):
                pend, lane = [], 0
                for _ in range((n_steps + 7) // 8):
                    if len(pend) == 2:
                        for h_ in pend.pop(0):
                            h_.result()
                    pend.append(m50.predict_batch_async(batch50, 0.05, lane=lane))
                    lane ^= 1
                while pend:
                    for h_ in pend.pop(0):
                        h_.result()
            steps_b = (args.steps + 7) // 8 * 8
            run50b(32)
            dt, _ = timed_median(run50b, steps_b, min(args.min_timed_seconds, 0.5))
            extra["resnet50_batch8_images_per_sec"] = round(steps_b / dt, 3)
            extra["resnet50_batch8_config"] = ("the same model and images as resnet50_images_per_sec as batches of 8 (model.predict_batch_async): one "
                                               "feature-extractor pass per batch, two batches in flight; default modes")
            set50(bottleneck_g3="off")
            run50b(32)
            dt, _ = timed_median(run50b, steps_b, min(args.min_timed_seconds, 0.5))
            extra["resnet50_batch8_f32_backbone_images_per_sec"] = round(steps_b / dt, 3)
            set50(**d50)
            m50._lanes.clear()
            del batch50
        except Exception as e:
            extra["resnet50_batch8_images_per_sec"] = {"error": "%s: %s" % (type(e).__name__, e)}
            set50(**d50)
        try:
            extra["resnet50_roofline"] = resnet_roofline_leg(m50, pool50[0], dev)
        except Exception as e:
            extra["resnet50_roofline"] = {"error": "%s: %s" % (type(e).__name__, e)}
        del m50, pool50
        # (3) the train step (row f3): the reference's fp32 RoIPool step, and configs[4]'s single-GPU form (bf16 gradient GEMMs, RoIAlign)
        extra["train_step_ms"] = {}
        for name, bb, kw in (("vgg16", "vgg16", {}), ("resnet101", "resnet101", {}),
                             ("vgg16_bf16", "vgg16", {"grad_math": "bf16"}),
                             ("resnet101_bf16_roialign", "resnet101", {"grad_math": "bf16", "roi_pooling": "align"})):
            try:
                extra["train_step_ms"][name] = train_step_leg(bb, dev, **kw)
            except Exception as e:     # a secondary leg must never take the headline line down with it
                extra["train_step_ms"][name] = {"error": "%s: %s" % (type(e).__name__, e)}
        torch.cuda.empty_cache()

    # ---- parity block and the host's cost per image (item 7), rank 0, outside the timed region -------------------
    parity = None
    host_us = None
    if rank == 0 and args.full and not is_resnet:
        try:
            parity = parity_leg(model, 0 if nslots == 1 else 1, synthetic.image, dev)
        except Exception as e:
            parity = {"error": "%s: %s" % (type(e).__name__, e)}
        # host CPU time of one predict_async (its ~33 launches, event records and the bookkeeping) while the GPU is kept busy: thread CPU time, so
        # waiting inside result() (a sleeping wait on the frame's event) does not count
        run(nslots)
        t_cpu, t_wall = time.thread_time(), time.perf_counter()
        n_host = 200
        pend = []
        t_submit = 0.0
        for i in range(n_host):
            if len(pend) == nslots:
                pend.pop(0).result()
            c0 = time.thread_time()
            pend.append(model.predict_async(pool[i % len(pool)], 0.05, slot=0 if nslots == 1 else 1 + (i % nslots)))
            t_submit += time.thread_time() - c0
        while pend:
            pend.pop(0).result()
        host_us = {"predict_async_submit_cpu_us": round(1e6 * t_submit / n_host, 1),
                   "submit_plus_result_cpu_us": round(1e6 * (time.thread_time() - t_cpu) / n_host, 1),
                   "wall_us_per_image": round(1e6 * (time.perf_counter() - t_wall) / n_host, 1),
                   "note": "host thread CPU time per image (time.thread_time) around predict_async alone and around predict_async + result(); 8 ranks on "
                           "one host need 8 x this per image-interval of CPU, against the wall time per image beside it"}

    # ---- mAP@0.5 leg (outside the timed region): labelled subset, merged across ranks -------------
    mean_ap = None
    if args.full:
        records = ImageRecords()
        for i in range(min(args.map_images, len(pool))):
            det = model.predict(pool[i], score_threshold=0.05)
            records.add(seeds[i], det, planted_ground_truth(seeds[i], det))
        calc = merged_calculator(records, force_gather=use_dist)       # ONE all-gather over RCCL when a process group is up
        mean_ap = float(calc.compute_mean_average_precision()) if calc._object_count_by_class_index else None

    out = None
    roofline = None
    if rank == 0 and args.full:
        # ---- roofline of the dominant kernel: HIP events around every conv3x3 MFMA launch, one stream
        # Per image: read + reset the per-class event sums, then keep the MEDIAN image per class (times its launch count), so
        # that one image hit by a clock ramp after the idle gap of the previous leg does not skew the mean.
        for i in range(3):
            model.predict(pool[i % len(pool)], score_threshold=0.05)
        ctx = model.context(0)
        ctx.timing_enable(True)
        per_image = []
        for i in range(max(args.roofline_images, 1)):
            model.predict(pool[i % len(pool)], score_threshold=0.05)
            torch.cuda.synchronize(dev)
            per_image.append(ctx.timing_read(reset=True))
        ctx.timing_enable(False)
        n_img = len(per_image)
        timing = {}
        for k in per_image[0]:
            ms = sorted(t[k][0] for t in per_image)
            med = ms[n_img // 2] if n_img % 2 else 0.5 * (ms[n_img // 2 - 1] + ms[n_img // 2])
            timing[k] = (med * n_img, sum(t[k][1] for t in per_image))     # (median image x images, launches)
        def mfma_roofline(kernel, cls, layer_flops, note):
            ms, launches = timing[cls]
            if not launches or not layer_flops:
                return None
            per_launch = float(sum(layer_flops)) / len(layer_flops)
            avg_s = (ms / 1e3) / launches
            ach = per_launch / avg_s / 1e12
            return {"kernel": kernel, "regime": regime, "bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_F32_MFMA_TFLOPS,
                    "unit": "TFLOP/s", "frac": round(ach / PEAK_F32_MFMA_TFLOPS, 4), "traffic": None, "flops_per_launch": per_launch,
                    "avg_launch_us": round(avg_s * 1e6, 2), "launches": int(launches), "ms_per_image": round(ms / max(args.roofline_images, 1), 4),
                    "note": note}

        # the tables SLOT 0 runs (this pass is one image at a time on slot 0): round 5 moves conv5_x / the RPN trunk to the one-launch form
        # there too (FasterRCNNModel.alone_winograd_x3f_layers)
        rx6, rx3, rx3f = (model.layer_tables(0) if not is_resnet else (x6, x3, x3f))
        regime = ("HIP events around every launch, one image at a time on one stream, median image of %d (after the timed region: with "
                  "several images in flight concurrent kernels share the CUs and a launch's wall duration is not its own)" % n_img)
        dl, wl_named = direct_layers(args.math, rx6), winograd_layers(args.math, rx6, named=True, x3f=rx3f)
        wl = [l for _, l in wl_named]
        xl_named = x6_winograd_layers(args.math, rx6, named=True)
        xl = [l for _, l in xl_named]
        r_direct = mfma_roofline("conv3x3_mfma_kernel (direct 3x3 layers: %d per image)" % len(dl), "conv3x3_mfma",
                                 [2.0 * 9 * ci * co * h * w for ci, co, h, w in dl], "FLOP = direct-convolution FLOP of the layers")
        if r_direct is not None:
            r_direct["traffic"] = measured_traffic()
        r_wino = mfma_roofline("wino_fused_kernel (one-launch float32 Winograd F(2x2,3x3) layer, all 16 positions in MFMA accumulators: %d layers "
                               "per image: %s)" % (len(wl), ", ".join(n for n, _ in wl_named)), "winograd_gemm", [winograd_gemm_flops(*l) for l in wl],
                               "FLOP = the FLOP the exact-f32 matrix pipe executes (16 x tiles x cin x cout x 2), NOT the 2.25x larger "
                               "direct-convolution FLOP the layers replace") if wl else None
        if r_wino is not None:
            r_wino["traffic"] = measured_traffic("wino_fused_kernel")
            prof = profiled_launch_us("wino_fused_kernel")
            if prof is not None:
                prof["frac"] = round(r_wino["flops_per_launch"] / (prof["mean_us"] * 1e-6) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)
                prof["note"] = "the committed rocprofv3 kernel-trace mean of the same single-stream regime (another box, another day): frac = flops_per_launch / mean / peak"
                r_wino["rocprof"] = prof
            r_wino["algorithmic_bytes_per_launch"] = float(sum(4.0 * (h * w * ci + 16 * ci * co + (h // (2 if n in _POOLED else 1)) * (w // (2 if n in _POOLED else 1)) * co)
                                                               for n, (ci, co, h, w) in wl_named)) / len(wl)
        if r_wino is not None and not args.no_extra_legs:
            try:
                r_wino["chip_full"] = winograd_chip_full_leg(wl_named, dev)
            except Exception as e:
                r_wino["chip_full"] = {"error": "%s: %s" % (type(e).__name__, e)}
        # the rx6 Winograd layers' batched GEMM on the bf16 pipe: executed FLOP = 6 x (16 x tiles x cin x cout x 2), priced against the
        # DENSE bf16 peak (the split-K reduction of the small maps is a separate, tiny launch in the same class: it is counted in the
        # class time but not in `launches`' FLOP, so the figure is slightly pessimistic)
        r_x6 = None
        if xl:
            ms6, l6 = timing["winograd_x6_gemm"]
            if l6:
                per_launch = sum((3.0 if n in rx3 else 6.0) * winograd_gemm_flops(*l) for n, l in xl_named) / len(xl)
                f32_eq = sum(winograd_gemm_flops(*l) for l in xl) / len(xl)
                n_gemm = len(xl) * n_img                               # GEMM launches (the class also holds the split-K reductions)
                avg_s = (ms6 / 1e3) / n_gemm
                ach = per_launch / avg_s / 1e12
                t8 = timing["winograd_x6_transforms"]
                r_x6 = {"kernel": "gemm_x6t_kernel / gemm_x3t_kernel (the 16 position GEMMs of a Winograd layer in one launch; f32x6 = six bf16 MFMAs per "
                                  "product: %s; f32x3 = three fp16 MFMAs per product: %s)"
                                  % (", ".join(n for n, _ in xl_named if n not in rx3) or "-", ", ".join(n for n, _ in xl_named if n in rx3) or "-"),
                        "regime": regime, "bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(ach / PEAK_BF16_MFMA_TFLOPS, 4), "traffic": measured_traffic("gemm_x3t_kernel" if rx3 else "gemm_x6t_kernel"),
                        "flops_per_launch": per_launch, "avg_launch_us": round(avg_s * 1e6, 2), "launches": int(n_gemm),
                        "ms_per_image": round(ms6 / max(args.roofline_images, 1), 4),
                        "f32_equivalent_tflops": round(f32_eq / avg_s / 1e12, 2),
                        "transforms_ms_per_image": round(t8[0] / max(args.roofline_images, 1), 4),
                        "algorithmic_bytes_per_launch": float(sum(16.0 * ((h + 1) // 2) * ((w + 1) // 2) * ((4 if n in rx3 else 6) * ci + 4 * co)
                                                                  + 16.0 * (4 if n in rx3 else 6) * ci * co for n, (ci, co, h, w) in xl_named)) / len(xl),
                        "note": "FLOP = 6 bf16 (f32x6) or 3 fp16 (f32x3) MFMA products per float32 product x the Winograd GEMM FLOP (16 x tiles x cin x "
                                "cout x 2), against the dense bf16 / fp16 peak (the same 2500 TFLOP/s); f32_equivalent_tflops = the same launches counted "
                                "once per float32 product; bytes = V records (6 / 4 B per element) read + M (4 B) written + the filter record bank"}
        # `roofline` = the kernel with the most GPU time per image, the other one rides along
        # the one-launch f32x3 Winograd layers (wino_x3d_kernel): 3 fp16 MFMAs per float32 product
        r_x3f = None
        fl_named = x3f_winograd_layers(args.math, rx6, rx3f)
        if fl_named and timing.get("winograd_x3f", (0, 0))[1]:
            msf, lf = timing["winograd_x3f"]
            per_launch = sum(3.0 * winograd_gemm_flops(*l) for _, l in fl_named) / len(fl_named)
            avg_s = (msf / 1e3) / lf
            ach = per_launch / avg_s / 1e12
            r_x3f = {"kernel": "wino_x3d_kernel (ONE-launch Winograd F(2x2,3x3) layer in the f32x3 arithmetic: operand formed in registers from the LDS-staged halo, "
                               "filter fragments straight from L2, all 16 positions in accumulators: %s; every producer leaves its output's channel maxima, "
                               "so no pass over a layer input remains in the class)"
                               % ", ".join(n for n, _ in fl_named),
                     "regime": regime, "bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(ach / PEAK_BF16_MFMA_TFLOPS, 4), "traffic": measured_traffic("wino_x3d_kernel"), "flops_per_launch": per_launch,
                     "avg_launch_us": round(avg_s * 1e6, 2), "launches": int(lf), "ms_per_image": round(msf / max(args.roofline_images, 1), 4),
                     "f32_equivalent_tflops": round(per_launch / 3.0 / avg_s / 1e12, 2),
                     "algorithmic_bytes_per_launch": float(sum(4.0 * (h * w * ci + 16 * ci * co + (h // (2 if n in _POOLED else 1)) * (w // (2 if n in _POOLED else 1)) * co)
                                                               for n, (ci, co, h, w) in fl_named)) / len(fl_named),
                     "note": "FLOP = 3 fp16 MFMA products per float32 product x the Winograd GEMM FLOP (16 x tiles x cin x cout x 2) against the dense fp16 peak; "
                             "f32_equivalent_tflops counts every float32 product once (the float32 one-launch kernel it replaces: ~100)"}
        both = [r for r in (r_direct, r_wino, r_x6, r_x3f) if r is not None]
        both.sort(key=lambda r: -r["ms_per_image"])
        roofline = dict(both[0]) if both else {"note": "timing disabled"}
        if len(both) > 1:
            roofline["second_kernel"] = both[1]
        if len(both) > 2:
            roofline["third_kernel"] = both[2]
        if len(both) > 3:
            roofline["fourth_kernel"] = both[3]
        roofline["per_class_ms_per_image"] = {k: round(v[0] / max(args.roofline_images, 1), 4) for k, v in timing.items()}
        # The same measurement for the table the HEADLINE runs (VERDICT r4 "do this" 5): the in-flight slots' arithmetic -- all 13 Winograd
        # layers in the one-launch f32x3 form -- one image at a time on slot 1's stream, so that a launch's duration is its own.
        if not is_resnet and nslots > 1 and args.math == "f32_winograd":
            try:
                for i in range(2):
                    model.predict_async(pool[i % len(pool)], 0.05, 1).result()
                ctx1 = model.context(1)
                ctx1.timing_enable(True)
                per1 = []
                for i in range(max(args.roofline_images, 1)):
                    model.predict_async(pool[i % len(pool)], 0.05, 1).result()
                    torch.cuda.synchronize(dev)
                    per1.append(ctx1.timing_read(reset=True))
                ctx1.timing_enable(False)
                n1 = len(per1)
                med1 = {}
                for k in per1[0]:
                    ms = sorted(t_[k][0] for t_ in per1)
                    med1[k] = (ms[n1 // 2] if n1 % 2 else 0.5 * (ms[n1 // 2 - 1] + ms[n1 // 2]), per1[0][k][1])
                hx6, hx3, hx3f = model.layer_tables(1)
                fl1 = x3f_winograd_layers(args.math, hx6, hx3f)
                msf1, lf1 = med1.get("winograd_x3f", (0.0, 0))
                if fl1 and lf1:
                    fl_sum = sum(3.0 * winograd_gemm_flops(*l) for _, l in fl1)
                    ach1 = fl_sum / (msf1 / 1e3) / 1e12
                    roofline["headline_table"] = {
                        "regime": "the arithmetic table of the in-flight slots (what `value` is measured on), one image at a time on slot 1's stream, "
                                  "HIP events around every launch, median image of %d" % n1,
                        "kernel": "wino_x3d_kernel: %s" % ", ".join(n_ for n_, _ in fl1), "launches_per_image": int(lf1),
                        "ms_per_image": round(msf1, 4), "avg_launch_us": round(msf1 * 1e3 / lf1, 2), "executed_gflop_per_image": round(fl_sum / 1e9, 2),
                        "achieved": round(ach1, 2), "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(ach1 / PEAK_BF16_MFMA_TFLOPS, 4),
                        "per_class_ms_per_image": {k: round(v[0], 4) for k, v in med1.items()}}
            except Exception as e:     # a secondary leg must never take the headline line down with it
                roofline["headline_table"] = {"error": "%s: %s" % (type(e).__name__, e)}
            try:
                roofline["per_layer"] = winograd_layer_fracs(dev)
            except Exception as e:
                roofline["per_layer"] = {"error": "%s: %s" % (type(e).__name__, e)}
        if is_resnet:
            roofline = {"note": "roofline block is defined for the VGG-16 headline workload only",
                        "per_class_ms_per_image": roofline["per_class_ms_per_image"]}

    if rank == 0:
        cpu = None
        if args.full and not args.no_cpu_baseline and n_gpus == 1 and not is_resnet:
            from oracle import frcnn_oracle as O       # CPU baseline leg only (checker, never the product)
            img0 = synthetic.image(seeds[0]).unsqueeze(0)
            cores = cpu_threads_for_baseline(sd, img0, O)
            O.predict(sd, img0, 0.05)                    # warm-up
            tc = time.perf_counter()
            for i in range(args.cpu_images):
                O.predict(sd, synthetic.image(seeds[i % len(seeds)]).unsqueeze(0), 0.05)
            dt = time.perf_counter() - tc
            cpu = {"value": round(args.cpu_images / dt, 4), "unit": "images/sec", "cores": cores, "kind": "port",
                   "sample": "%d x predict() of the 600x1000 workload through oracle/frcnn_oracle.py "
                             "(torch-CPU conv/linear; best of several thread counts = %d of %d host cores), %.1f s" % (
                                 args.cpu_images, cores, os.cpu_count() or 1, dt)}

        # algorithmic FLOP per image: VGG-16 from the layer shapes, ResNets from BASELINE.md section 3
        flops_img = {"vgg16": total_flops_per_image(), "resnet50": 2.7845e11, "resnet101": 3.6913e11,
                     "resnet152": 4.5937e11}[args.backbone]
        pipes = {}
        if not is_resnet:
            ips = value / n_gpus
            # the tables the HEADLINE ran on: with images in flight the 512-channel f32x3 layers take the one-launch form (FasterRCNNModel.layer_tables)
            hx6, hx3, hx3f = model.layer_tables(0 if nslots == 1 else 1)
            pf = pipe_flops_per_image(args.math, fc_math, hx6, x3=hx3, x3f=hx3f)
            pb = pipe_flops_per_image(args.math, fc_math, hx6, backbone_only=True, x3=hx3, x3f=hx3f)
            f32_tf, bf16_tf, f16_tf = ips * pf["f32"] / 1e12, ips * pf["bf16"] / 1e12, ips * pf["f16"] / 1e12
            pipes = {
                "layer_arithmetic": [{"layer": n_, "kernel": k_, "pipe": p_, "executed_gflop": round(e_ / 1e9, 3), "algorithmic_gflop": round(a_ / 1e9, 3)}
                                     for n_, k_, p_, e_, a_ in layer_arithmetic(args.math, fc_math, hx6, x3=hx3, x3f=hx3f)],
                "layer_arithmetic_note": "the kernels of the headline's %d-images-in-flight slots; one image at a time (slot 0, the regime of the `roofline` "
                                         "block) runs %s as three-launch f32x3 layers instead (same arithmetic up to the rounding order of the output transform)"
                                         % (nslots, ", ".join(n_ for n_ in hx3f if n_ not in x3f) or "-"),
                "f32_pipe_tflops": round(f32_tf, 2), "f32_pipe_frac": round(f32_tf / PEAK_F32_MFMA_TFLOPS, 4),
                "bf16_pipe_tflops": round(bf16_tf, 2), "bf16_pipe_frac": round(bf16_tf / PEAK_BF16_MFMA_TFLOPS, 4),
                "f16_pipe_tflops": round(f16_tf, 2), "f16_pipe_frac": round(f16_tf / PEAK_BF16_MFMA_TFLOPS, 4),
                "pipe_note": "FLOP each kind of matrix instruction EXECUTES per image x images/sec per GPU, over its dense peak (float32 MFMA 157.3, bf16 "
                             "and fp16 MFMA 2500 TFLOP/s each); they share the SIMDs' MFMA issue, so the fractions add up to the matrix-unit busy "
                             "fraction the workload needs at peak rate.  bf16 = the f32x6 layers (six MFMAs per float32 product), f16 = the f32x3 layers "
                             "(three)",
                # "fraction of conv roofline" = backbone(+RPN trunk) 3x3 conv FLOP x images/sec / MFMA peak, per pipe
                "conv_roofline_frac": round(ips * pb["f32"] / 1e12 / PEAK_F32_MFMA_TFLOPS + ips * (pb["bf16"] + pb["f16"]) / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4),
                "conv_roofline_note": "EXECUTED 3x3-conv FLOP (conv1_2 .. conv5_3 + RPN trunk; Winograd layers count 16 x tiles x cin x cout x 2) x images/sec "
                                      "per GPU / the peak of the pipe each layer runs on, summed; direct-form FLOP (3.75e11 per image) would give %.4f of the f32 peak"
                                      % (ips * conv_mfma_flops_per_image() / 1e12 / PEAK_F32_MFMA_TFLOPS),
                "mfma_tflops_executed_per_gpu": round(f32_tf + bf16_tf + f16_tf, 2),
                "mfma_tflops_executed_note": "sum over ALL matrix instruction kinds (kept for continuity with rounds 1-2); read f32_ / bf16_ / f16_pipe_tflops instead",
            }
        # the arithmetic, said where `dtype` is read: tensors are float32 everywhere; the split-operand layers are NOT float32
        # operand arithmetic (f32x3 keeps 22-23 bits of an operand relative to its row's / tile's largest element)
        n_x3 = len([n_ for n_ in x6 if n_ in x3]) + len(x3f) + (2 if fc_math == "f32x3" else 0)
        n_x6 = len([n_ for n_ in x6 if n_ not in x3]) + (2 if fc_math == "f32x6" else 0)
        if is_resnet or (n_x3 == 0 and n_x6 == 0):
            dtype_str = "f32" if not is_resnet else "f32 (ResNet: layer4 / RPN trunk GEMMs in the model's default split-operand arithmetic, f32 accumulation)"
        else:
            dtype_str = ("f32 (float32 tensors and accumulation; %d GEMM layers in the f32x3 split-operand emulation = two fp16 terms per block-scaled operand, "
                         "three fp16 MFMAs per product; %d in f32x6 = three bf16 terms, six bf16 MFMAs; the other %d on exact-f32 MFMA; "
                         "strict exact-f32 everywhere: config.strict_f32_images_per_sec)" % (n_x3, n_x6, 17 - n_x3 - n_x6))
        out = {
            "metric": "images/sec (600x1000) Faster-RCNN %s inference" % ("VGG-16" if not is_resnet else args.backbone), "value": round(value, 3),
            "unit": "images/sec", "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup, "ramp_seconds": args.ramp_seconds,
            "ms_per_step": round(1e3 * elapsed / args.steps, 4),
            "timed_bursts": {"count": len(bursts), "reported": "median burst of `steps` steps", "min_ms": round(1e3 * min(bursts), 3),
                             "max_ms": round(1e3 * max(bursts), 3), "total_timed_s": round(sum(bursts), 3)},
            "full": args.full, "rocm_smi_under_load": smi, "process_group": ("nccl x%d" % world) if use_dist else None, "world_size": world, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": dtype_str, "data": "synthetic",
            "config": {"workload": ("VGG-16" if not is_resnet else args.backbone) + " Faster R-CNN predict(), 3x600x1000 float32, batch=1 per forward, "
                                   "6000 pre-/300 post-NMS proposals, score_threshold 0.05",
                       "images_in_flight_per_gpu": nslots, "hip_hw_queues": hw_queues(), "parallelism": "image-parallel x%d" % n_gpus,
                       "flops_per_image": flops_img,
                       # the same workload, same run: every GEMM on the exact-f32 matrix instructions / fed from pinned host memory
                       "strict_f32_images_per_sec": strict_f32_value,
                       "h2d_preprocess_images_per_sec": h2d.get("h2d_preprocess_images_per_sec"),
                       "h2d_float32_images_per_sec": h2d.get("h2d_float32_images_per_sec")},
            "tflops_per_gpu": round(value / n_gpus * flops_img / 1e12, 2),
            "tflops_per_gpu_note": "direct-convolution FLOP of the workload x images/sec (BASELINE.md's 4.4922e11 per image); "
                                   "in the f32_winograd mode the matrix pipes execute fewer: see f32_pipe_tflops / bf16_pipe_tflops",
            "math": args.math, "winograd_x6_layers": list(x6), "winograd_x3_layers": list(x3), "winograd_x3f_layers": list(x3f), "inflight_winograd_x3f_layers": [] if is_resnet else list(model.inflight_winograd_x3f_layers), "fc_math": None if is_resnet else fc_math, "roi": model._stage3_detector_network.pooling,
            "other_math_modes_images_per_sec": secondary, "fc_math_f32_images_per_sec": fc_f32_value,
            "winograd_all_f32_pipe_images_per_sec": wino_f32_value, "strict_f32_images_per_sec": strict_f32_value,
            **h2d,
            **x3_legs,
            "per_rank_images_per_sec": per_rank, "slowest_rank_images_per_sec": min(per_rank) if per_rank else None,
            **pipes,
            **extra,
            "map_at_0.5": mean_ap, "map_images": int(args.map_images * world) if args.full else 0,
            "map_note": "plumbing check, not accuracy: random-init weights; the ground truth of each labelled image is seeded random boxes plus up "
                        "to 3 of the model's OWN top detections jittered by a few pixels, so the value only shows that predict -> per-image "
                        "records -> (all-gather) -> AP integration runs end to end and is reproducible; README.md:38's mAP needs trained weights",
            "parity": parity, "host_cpu_per_image": host_us,
            "roofline": roofline, "cpu_baseline": cpu,
        }
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    return out


if __name__ == "__main__":
    main()

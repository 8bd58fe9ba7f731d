"""tools/nms_band.py -- the chunk at which nms_reduce_kernel (csrc/proposals.hip) keeps its last proposal, over the images NMS_BAND is
chosen from: the golden 600x1000 image, every tests/golden/holdout/vgg16_*_w1234.npz image and bench.py's eight pool images.  Prints one
line per image (candidates, kept, chunks resolved, whether phase B's reduce ran, i.e. the `done` word read 0 behind phase A) and the
band the rule gives: the smallest multiple of 8 that is >= 1.5 x the largest stopping chunk.
Needs a library built with -DNMS_CLOCKS:  SRC=proposals tools/build_ablate.sh nmsclk -DNMS_CLOCKS ; FRCNN_LIB_PATH=build/libfrcnn_nmsclk.so
(the kernel leaves its clocks and these counts in the last four proposals: the forward's results are wrong in that build)."""
import glob
import os
import sys
import numpy as np
import torch
sys.path.insert(0, ".")
from fasterrcnn_amd import synthetic
from fasterrcnn_amd.models.faster_rcnn import FasterRCNNModel
from fasterrcnn_amd.models.vgg16 import VGG16Backbone

model = FasterRCNNModel(num_classes=21, backbone=VGG16Backbone(dropout_probability=0.0))
model.load_state_dict(synthetic.vgg16_state_dict(1234), strict=True)
model = model.cuda().eval()

images = [("golden s0", synthetic.image(0, 600, 1000))]
for f in sorted(glob.glob(os.path.join("tests", "golden", "holdout", "vgg16_*_w1234.npz"))):
    g = np.load(f)
    images.append(("holdout s%d" % int(g["seed"]), synthetic.image(int(g["seed"]), int(g["height"]), int(g["width"]))))
images += [("bench pool %d" % s, synthetic.image(s)) for s in range(8)]

worst, fallbacks = 0, 0
for name, img in images:
    p, _, _ = model(image_data=img.unsqueeze(0).cuda())
    torch.cuda.synchronize()
    b, c, d = p[-2].tolist(), p[-3].tolist(), p[-4].tolist()
    c_done, fell_back = int(b[3]), int(d[0])
    worst, fallbacks = max(worst, c_done), fallbacks + fell_back
    print("%-14s %4dx%-4d: %d candidates, %d kept, %d chunks resolved, launch limit %d, phase B %s"
          % (name, img.shape[-2], img.shape[-1], c[2], c[3], c_done, int(d[1]), "RAN" if fell_back else "did not run"))
band = -(-int(np.ceil(1.5 * worst)) // 8) * 8
print("%d images: largest stopping chunk %d -> NMS_BAND = %d; phase B ran on %d images" % (len(images), worst, band, fallbacks))

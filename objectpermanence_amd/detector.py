"""Detector front-end on MI355X - mirror of reference baselines/detector.py (CaterObjectDetector) and
object_detection/models.py:6-20: torchvision's fasterrcnn_resnet50_fpn (193 classes) in eval mode - frame
preprocessing, the ResNet-50-FPN backbone, the RPN head, TwoMLPHead and FastRCNNPredictor on the MFMA conv/GEMM
kernels (conv_kernels.hip), proposal selection, MultiScaleRoIAlign and detection post-processing on
det_head_kernels.hip.

PARITY UNPINNED: torchvision 0.5.0 and the fine-tuned weights are absent, so everything
is checked against a build-authored restatement (oracle/detector_oracle.py), not against the reference's
detector.  ``CaterObjectDetector.__call__`` returns what detector.py:84 returns: ``[{"boxes", "labels", "scores"}]``.
"""
from __future__ import annotations

import ctypes
import collections
import os
from collections import OrderedDict
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _lib

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
_LAYERS = (3, 4, 6, 3)


# passes a caller keeps enqueued at once on alternating streams (preprocess_perception_main, bench.py): the partial last round of one
# pass's conv launches is filled by the next pass's workgroups
PASSES_IN_FLIGHT = 3


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# (device, stream) -> workspace of the Winograd convs enqueued on that stream, most recently used last; at most _WINO_WS_MAX of them
# are kept (a workspace is allocated on the stream it is used on, so dropping one is stream-ordered like any torch free)
_WINO_WS: "collections.OrderedDict[tuple, torch.Tensor]" = collections.OrderedDict()
_WINO_WS_MAX = max(1, int(os.environ.get("OPDET_WINO_WS_STREAMS", "4")))


class _Conv:
    """one conv (+ folded FrozenBatchNorm) packed for opdet_conv2d_f32: weight [Cout][KP], k = (dy*KW+dx)*Cin + ci"""

    def __init__(self, sd, wname: str, bn: str = None, bias: str = None, stride=1, pad=0, bn_eps=0.0, device="cuda:0"):
        w = torch.as_tensor(sd[wname], dtype=torch.float32)
        cout, cin, kh, kw = w.shape
        b = torch.zeros(cout) if bias is None else torch.as_tensor(sd[bias], dtype=torch.float32).clone()
        if bn is not None:
            g, beta = torch.as_tensor(sd[bn + ".weight"]).float(), torch.as_tensor(sd[bn + ".bias"]).float()
            rm, rv = torch.as_tensor(sd[bn + ".running_mean"]).float(), torch.as_tensor(sd[bn + ".running_var"]).float()
            scale = g / torch.sqrt(rv + bn_eps)
            w = w * scale[:, None, None, None]
            b = beta - rm * scale
        cin_p = (cin + 3) // 4 * 4                     # stem: 3 -> 4 channels
        wp = torch.zeros((cout, kh, kw, cin_p))
        wp[..., :cin] = w.permute(0, 2, 3, 1)
        k = kh * kw * cin_p
        self.kp = (k + 15) // 16 * 16
        packed = torch.zeros((cout, self.kp))
        packed[:, :k] = wp.reshape(cout, k)
        self.w = packed.contiguous().to(device)
        self.b = b.contiguous().to(device)
        self.cin, self.cout, self.kh, self.kw, self.stride, self.pad = cin_p, cout, kh, kw, stride, pad
        self._ws_bytes: Dict[tuple, int] = {}
        self._u = None                  # Winograd-transformed weights [16][Cout][Cin], made on first use

    # Winograd F(2 x 2, 3 x 3) (csrc/wino_kernels.hip) for the stride-1 3 x 3 convs with >= WINO_MIN_CIN input channels and at least
    # WINO_MIN_TILES 2 x 2 output tiles in the call: 2.25 x fewer MACs against 4 x the activation traffic - measured 1.26 x on the
    # P2-level 256 -> 256 conv of a 16-frame pass, results within 2.2e-6 of max|y| of the direct conv (profiles/r6_winograd_probe.txt).
    # OPDET_WINOGRAD=0 keeps every conv direct.
    WINO_MIN_CIN = int(os.environ.get("OPDET_WINO_MIN_CIN", "256"))
    WINO_MIN_TILES = int(os.environ.get("OPDET_WINO_MIN_TILES", "200"))

    def _winograd(self, n: int, h: int, w: int, residual) -> bool:
        return (os.environ.get("OPDET_WINOGRAD", "1") != "0" and residual is None and self.kh == 3 and self.kw == 3 and self.stride == 1
                and self.pad == 1 and self.cin % 16 == 0 and self.cout % 4 == 0 and self.cin >= self.WINO_MIN_CIN
                and n * ((h + 1) // 2) * ((w + 1) // 2) >= self.WINO_MIN_TILES)

    def _call_winograd(self, x: torch.Tensor, relu: bool) -> torch.Tensor:
        lib = _lib.load()
        n, h, w, c = x.shape
        st = _stream(x.device)
        if self._u is None or self._u.device != x.device:
            u = torch.empty(int(lib.opdet_wino_weights_bytes(c, self.cout)) // 4, dtype=torch.float32, device=x.device)
            _lib.check(lib.opdet_wino_weights_f32(self.w.data_ptr(), u.data_ptr(), c, self.cout, self.kp, st), "opdet_wino_weights_f32")
            # the transformed weights are shared by every stream that runs this conv, with no event between them: they are complete
            # before they are published (once per weight set; without the wait the second pass in flight - on another stream - of a
            # fresh detector multiplied by weights that the first pass's stream had not transformed yet)
            torch.cuda.current_stream(x.device).synchronize()
            self._u = u
        y = torch.empty((n, h, w, self.cout), dtype=torch.float32, device=x.device)
        key = ("wino", n, h, w)
        nws = self._ws_bytes.get(key)
        if nws is None:
            nws = self._ws_bytes[key] = int(lib.opdet_conv2d_wino_workspace_bytes(n, h, w, c, self.cout))
        # ONE grow-only workspace per (device, stream): the Winograd convs of a stream run one after the other, and fresh multi-GB
        # blocks from the caching allocator inside a pass stall it (measured: 220 against 380 frames/s when three passes in flight
        # each allocated theirs in the timed region)
        wkey = (x.device, st)
        ws = _WINO_WS.get(wkey)
        if ws is None or ws.numel() < nws:
            _WINO_WS.pop(wkey, None)
            while len(_WINO_WS) >= _WINO_WS_MAX:
                _WINO_WS.popitem(last=False)
            ws = _WINO_WS[wkey] = torch.empty(nws, dtype=torch.uint8, device=x.device)
        else:
            _WINO_WS.move_to_end(wkey)
        rc = lib.opdet_conv2d_wino_f32(x.data_ptr(), self._u.data_ptr(), self.b.data_ptr(), y.data_ptr(), n, h, w, c, self.cout, int(relu),
                                       ws.data_ptr(), ws.numel(), st)
        _lib.check(rc, "opdet_conv2d_wino_f32")
        return y

    def __call__(self, x: torch.Tensor, relu: bool, residual: torch.Tensor = None) -> torch.Tensor:
        lib = _lib.load()
        n, h, w, c = x.shape
        assert c == self.cin, (c, self.cin)
        if self._winograd(n, h, w, residual):
            return self._call_winograd(x, relu)
        oh = (h + 2 * self.pad - self.kh) // self.stride + 1
        ow = (w + 2 * self.pad - self.kw) // self.stride + 1
        y = torch.empty((n, oh, ow, self.cout), dtype=torch.float32, device=x.device)
        shape = (n, h, w, c, self.cout, self.kh, self.kw, self.stride, self.pad, self.kp)
        nws = self._ws_bytes.get(shape)
        if nws is None:                 # > 0: too few output tiles for 256 CUs (one frame's deep maps, the FCs) - K is split
            nws = self._ws_bytes[shape] = int(lib.opdet_conv2d_workspace_bytes(*shape))
        ws = torch.empty(nws, dtype=torch.uint8, device=x.device) if nws else None       # (caching allocator: stream-ordered reuse)
        rc = lib.opdet_conv2d_ws_f32(x.data_ptr(), self.w.data_ptr(), self.b.data_ptr(),
                                     None if residual is None else residual.data_ptr(), y.data_ptr(), *shape, int(relu),
                                     None if ws is None else ws.data_ptr(), nws, _stream(x.device))
        _lib.check(rc, "opdet_conv2d_ws_f32")
        return y

    def plus_upsampled(self, x: torch.Tensor, top: torch.Tensor) -> torch.Tensor:
        """conv(x) + bias + F.interpolate(top, size=conv's, mode="nearest"): FeaturePyramidNetwork's top-down step in one call"""
        lib = _lib.load()
        n, h, w, c = x.shape
        assert c == self.cin and top.shape[0] == n and top.shape[3] == self.cout and top.is_contiguous()
        oh = (h + 2 * self.pad - self.kh) // self.stride + 1
        ow = (w + 2 * self.pad - self.kw) // self.stride + 1
        y = torch.empty((n, oh, ow, self.cout), dtype=torch.float32, device=x.device)
        shape = (n, h, w, c, self.cout, self.kh, self.kw, self.stride, self.pad, self.kp)
        nws = self._ws_bytes.get(shape)
        if nws is None:
            nws = self._ws_bytes[shape] = int(lib.opdet_conv2d_workspace_bytes(*shape))
        ws = torch.empty(nws, dtype=torch.uint8, device=x.device) if nws else None
        rc = lib.opdet_conv2d_up_f32(x.data_ptr(), self.w.data_ptr(), self.b.data_ptr(), top.data_ptr(), y.data_ptr(), *shape,
                                     int(top.shape[1]), int(top.shape[2]), None if ws is None else ws.data_ptr(), nws,
                                     _stream(x.device))
        _lib.check(rc, "opdet_conv2d_up_f32")
        return y


class _DualConv:
    """conv3 + downsample of a stage's first bottleneck (both 1 x 1, FrozenBN folded) as ONE product over the concatenated K:
    relu(conv3(out) + downsample(x)) without the downsample's output ever being written.  Shapes the LDS-DMA kernel does not run
    (tiny maps) go through the two convs."""

    def __init__(self, c3: _Conv, ds: _Conv):
        assert (c3.kh, c3.kw, ds.kh, ds.kw, c3.stride, c3.pad, ds.pad) == (1, 1, 1, 1, 1, 0, 0) and c3.cout == ds.cout
        self.c3, self.ds = c3, ds
        self.ok = c3.cin % 16 == 0 and ds.cin % 16 == 0 and c3.cout % 4 == 0
        if self.ok:
            self.w = torch.cat([c3.w[:, :c3.cin], ds.w[:, :ds.cin]], dim=1).contiguous()
            self.b = (c3.b + ds.b).contiguous()
        self._ws_bytes: Dict[tuple, int] = {}

    def __call__(self, out: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        c3, ds = self.c3, self.ds
        n, h, w, _ = out.shape
        shape = (n, h, w, c3.cin, int(x.shape[1]), int(x.shape[2]), ds.cin, ds.stride, c3.cout)
        lib = _lib.load()
        nws = self._ws_bytes.get(shape)
        if nws is None:
            nws = self._ws_bytes[shape] = int(lib.opdet_conv2d_dual_workspace_bytes(*shape)) if self.ok else -1
        if nws < 0:
            return c3(out, relu=True, residual=ds(x, relu=False))
        y = torch.empty((n, h, w, c3.cout), dtype=torch.float32, device=out.device)
        ws = torch.empty(nws, dtype=torch.uint8, device=out.device) if nws else None
        rc = lib.opdet_conv2d_dual_f32(out.data_ptr(), x.data_ptr(), self.w.data_ptr(), self.b.data_ptr(), y.data_ptr(), *shape, 1,
                                       None if ws is None else ws.data_ptr(), nws, _stream(out.device))
        _lib.check(rc, "opdet_conv2d_dual_f32")
        return y


class _Linear(_Conv):
    """nn.Linear as a 1x1 "conv" over a row of R pixels: x [R, K] -> [R, out]"""

    def __init__(self, weight: torch.Tensor, bias: torch.Tensor, device):
        out_f, in_f = weight.shape
        super().__init__({"w": weight.reshape(out_f, in_f, 1, 1), "b": bias}, "w", bias="b", device=device)

    def rows(self, x: torch.Tensor, relu: bool) -> torch.Tensor:
        r, k = x.shape
        return super().__call__(x.view(1, 1, r, k), relu=relu).view(r, self.cout)


class FasterRCNNHeads:
    """model.rpn + model.roi_heads + the box half of model.transform.postprocess of fasterrcnn_resnet50_fpn
    (eval mode), on NHWC FPN maps.  Defaults are torchvision's (faster_rcnn.py: rpn_pre/post_nms_top_n_test 1000,
    rpn_nms_thresh 0.7, box_score_thresh 0.05, box_nms_thresh 0.5, box_detections_per_img 100)."""

    ANCHOR_SIZES = (32, 64, 128, 256, 512)

    def __init__(self, state_dict, device="cuda:0", num_classes: int = 193, pre_nms_top_n: int = 1000,
                 post_nms_top_n: int = 1000, rpn_nms_thresh: float = 0.7, score_thresh: float = 0.05,
                 nms_thresh: float = 0.5, detections_per_img: int = 100):
        sd = {k: torch.as_tensor(v, dtype=torch.float32) for k, v in state_dict.items()
              if k.startswith("rpn.") or k.startswith("roi_heads.")}
        self.device = torch.device(device)
        self.rpn_conv = _Conv(sd, "rpn.head.conv.weight", bias="rpn.head.conv.bias", pad=1, device=device)
        # cls_logits (3) and bbox_pred (12) as ONE 1x1 conv with 16 output channels: [obj x3 | deltas x12 | 0]
        w = torch.zeros((16, 256, 1, 1))
        b = torch.zeros(16)
        w[0:3], w[3:15] = sd["rpn.head.cls_logits.weight"], sd["rpn.head.bbox_pred.weight"]
        b[0:3], b[3:15] = sd["rpn.head.cls_logits.bias"], sd["rpn.head.bbox_pred.bias"]
        self.rpn_out = _Conv({"w": w, "b": b}, "w", bias="b", device=device)
        # fc6 consumes the pooled map flattened as (C,7,7); the HIP RoIAlign writes (7,7,C): permute the columns once
        w6 = sd["roi_heads.box_head.fc6.weight"]
        c = w6.shape[1] // 49
        w6 = w6.view(-1, c, 7, 7).permute(0, 2, 3, 1).reshape(w6.shape[0], -1)
        self.fc6 = _Linear(w6, sd["roi_heads.box_head.fc6.bias"], device)
        self.fc7 = _Linear(sd["roi_heads.box_head.fc7.weight"], sd["roi_heads.box_head.fc7.bias"], device)
        # FastRCNNPredictor's two Linears (cls_score NC, bbox_pred 4 NC) as ONE product: output row = [scores | pad to a multiple of
        # 4 | deltas]; the detections stage reads the two parts through row strides
        wc, wb = sd["roi_heads.box_predictor.cls_score.weight"], sd["roi_heads.box_predictor.bbox_pred.weight"]
        if wc.shape[0] != num_classes or wb.shape[0] != 4 * num_classes:
            raise ValueError("box predictor shape does not match num_classes")
        self._reg_col = (num_classes + 3) // 4 * 4
        w = torch.zeros((self._reg_col + 4 * num_classes, wc.shape[1]))
        b = torch.zeros(self._reg_col + 4 * num_classes)
        w[:num_classes], w[self._reg_col:] = wc, wb
        b[:num_classes], b[self._reg_col:] = sd["roi_heads.box_predictor.cls_score.bias"], sd["roi_heads.box_predictor.bbox_pred.bias"]
        self.predictor = _Linear(w, b, device)
        self.num_classes = num_classes
        self.pre_nms_top_n, self.post_nms_top_n, self.rpn_nms_thresh = pre_nms_top_n, post_nms_top_n, rpn_nms_thresh
        self.score_thresh, self.nms_thresh, self.detections_per_img = score_thresh, nms_thresh, detections_per_img
        self._ws: Dict[tuple, torch.Tensor] = {}

    def _workspace(self, key, nbytes: int, what: str) -> torch.Tensor:
        if nbytes == 0:
            _lib.check(-2, what)
        key = key + (_stream(self.device),)              # one workspace per (shape, stream): images overlap on side streams
        if key not in self._ws:
            self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws[key]

    def rpn_head(self, feats: "OrderedDict[str, torch.Tensor]") -> List[torch.Tensor]:
        """RPNHead on the five maps -> [n, h, w, 16] each (objectness x3, deltas x12, pad)"""
        return [self.rpn_out(self.rpn_conv(f, relu=True), relu=False) for f in feats.values()]

    def proposals(self, head_outs: List[torch.Tensor], image_size, padded_size):
        """RegionProposalNetwork.filter_proposals for the n equally sized images of head_outs ([n, h, w, 16] per level), one launch per
        stage: -> (proposals [n, post, 4], scores [n, post], count [n] int32)"""
        lib = _lib.load()
        dev = self.device
        nl = len(head_outs)
        n = int(head_outs[0].shape[0])
        IntArr, PtrArr = ctypes.c_int * nl, ctypes.c_void_p * nl
        for h in head_outs:
            if h.shape[0] != n or h.shape[3] != 16 or not h.is_contiguous():
                raise ValueError("head outputs must be contiguous [n, h, w, 16]")
        gh, gw = IntArr(*[int(h.shape[1]) for h in head_outs]), IntArr(*[int(h.shape[2]) for h in head_outs])
        sizes = IntArr(*self.ANCHOR_SIZES[:nl])
        ptrs = PtrArr(*[h.data_ptr() for h in head_outs])
        ph, pw = int(padded_size[0]), int(padded_size[1])
        key = ("rpn", n, tuple(gh), tuple(gw), ph, pw)
        ws = self._workspace(key, lib.opdet_rpn_workspace_bytes_batch(n, nl, gh, gw, sizes, ph, pw, self.pre_nms_top_n),
                             "opdet_rpn_workspace_bytes_batch")
        props = torch.empty((n, self.post_nms_top_n, 4), dtype=torch.float32, device=dev)
        scores = torch.empty((n, self.post_nms_top_n), dtype=torch.float32, device=dev)
        count = torch.empty((n,), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.opdet_rpn_proposals_batch_f32(ptrs, n, nl, gh, gw, sizes, int(image_size[0]), int(image_size[1]), ph, pw,
                                                   self.pre_nms_top_n, self.post_nms_top_n, self.rpn_nms_thresh, 1e-3,
                                                   props.data_ptr(), scores.data_ptr(), count.data_ptr(), ws.data_ptr(),
                                                   ws.numel(), _stream(dev))
        _lib.check(rc, "opdet_rpn_proposals_batch_f32")
        return props, scores, count

    def roi_align(self, feats: List[torch.Tensor], props: torch.Tensor, count: torch.Tensor, image_size,
                  out: torch.Tensor = None) -> torch.Tensor:
        """MultiScaleRoIAlign on maps "0".."3" ([n, h, w, C] each) with props [n, R, 4], count [n] -> [n * R, 7, 7, C]"""
        lib = _lib.load()
        IntArr, PtrArr = ctypes.c_int * 4, ctypes.c_void_p * 4
        n = int(feats[0].shape[0])
        if props.dim() == 2:
            props = props[None]
        if props.dim() != 3 or props.shape[0] != n or count.numel() != n or any(f.shape[0] != n or not f.is_contiguous() for f in feats[:4]):
            raise ValueError("roi_align: maps [n, h, w, C], props [n, R, 4], count [n]")
        fh, fw = IntArr(*[int(f.shape[1]) for f in feats[:4]]), IntArr(*[int(f.shape[2]) for f in feats[:4]])
        ptrs = PtrArr(*[f.data_ptr() for f in feats[:4]])
        c = int(feats[0].shape[3])
        r = int(props.shape[1])
        if out is None:
            out = torch.empty((n * r, 7, 7, c), dtype=torch.float32, device=props.device)
        with torch.cuda.device(props.device):
            rc = lib.opdet_roi_align_batch_f32(ptrs, n, fh, fw, c, int(image_size[0]), props.data_ptr(), count.data_ptr(), r,
                                               out.data_ptr(), _stream(props.device))
        _lib.check(rc, "opdet_roi_align_batch_f32")
        return out

    def box_heads(self, pooled: torch.Tensor):
        """TwoMLPHead + FastRCNNPredictor -> (class_logits [R, NC], box_regression [R, 4 NC]): two column ranges of one product"""
        x = self.fc7.rows(self.fc6.rows(pooled.view(pooled.shape[0], -1), relu=True), relu=True)
        both = self.predictor.rows(x, relu=False)
        return both[:, :self.num_classes], both[:, self._reg_col:]

    def detections(self, class_logits, box_regression, props, count, image_size, original_size):
        """RoIHeads.postprocess_detections + rescale for n images: class_logits [n * R, NC], box_regression [n * R, 4 NC], props
        [n, R, 4], count [n] -> boxes [n, md, 4], scores [n, md], labels [n, md] int64, n_det [n] int32"""
        lib = _lib.load()
        dev = props.device
        if props.dim() == 2:
            props = props[None]
        n, r, nc, md = int(props.shape[0]), int(props.shape[1]), self.num_classes, self.detections_per_img
        if class_logits.shape[0] != n * r or box_regression.shape[0] != n * r or class_logits.stride(1) != 1 or box_regression.stride(1) != 1:
            raise ValueError("detections: class_logits / box_regression must have n * R rows of unit-stride columns")
        ws = self._workspace(("det", n, r, nc), lib.opdet_detections_workspace_bytes_batch(n, r, nc),
                             "opdet_detections_workspace_bytes_batch")
        boxes = torch.empty((n, md, 4), dtype=torch.float32, device=dev)
        scores = torch.empty((n, md), dtype=torch.float32, device=dev)
        labels = torch.empty((n, md), dtype=torch.int64, device=dev)
        n_det = torch.empty((n,), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.opdet_detections_batch_f32(class_logits.data_ptr(), box_regression.data_ptr(), props.data_ptr(),
                                                count.data_ptr(), n, r, nc, int(class_logits.stride(0)), int(box_regression.stride(0)),
                                                int(image_size[0]), int(image_size[1]),
                                                int(original_size[0]), int(original_size[1]), self.score_thresh,
                                                self.nms_thresh, md, boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(),
                                                n_det.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev))
        _lib.check(rc, "opdet_detections_batch_f32")
        return boxes, scores, labels, n_det

    def forward_images(self, feats: "OrderedDict[str, torch.Tensor]", image_sizes, padded_size, original_sizes):
        """feats: the five maps of n images ([n,h,w,256]).  Every stage - the dense ones (RPN head, TwoMLPHead, predictors) and the
        selection ones (proposals, RoIAlign, detections) - is launched ONCE for all the images of a run that share (resized size,
        original size): the frames of a video do, so a pass is one run (reference detector.py:84 calls the model per frame).
        -> list of padded (boxes [md,4], scores [md], labels [md], n_det [1]) per image"""
        outs = [None] * int(next(iter(feats.values())).shape[0])
        for (a, b), (boxes, scores, labels, n_det) in self.forward_runs(feats, image_sizes, padded_size, original_sizes):
            for i in range(a, b):
                outs[i] = (boxes[i - a], scores[i - a], labels[i - a], n_det[i - a:i - a + 1])
        return outs

    def forward_runs(self, feats: "OrderedDict[str, torch.Tensor]", image_sizes, padded_size, original_sizes):
        """forward_images' work, its results per run: -> list of ((a, b), (boxes [b-a,md,4], scores [b-a,md], labels [b-a,md],
        n_det [b-a])) for the maximal runs [a, b) of images with one geometry"""
        n = int(next(iter(feats.values())).shape[0])
        head = self.rpn_head(feats)
        maps = list(feats.values())
        r = self.post_nms_top_n
        sizes = [(tuple(int(v) for v in image_sizes[i]), tuple(int(v) for v in original_sizes[i])) for i in range(n)]
        runs = []           # maximal runs of consecutive images with one geometry
        for i in range(n):
            if runs and sizes[runs[-1][0]] == sizes[i]:
                runs[-1][1] = i + 1
            else:
                runs.append([i, i + 1])
        whole = len(runs) == 1
        pooled = torch.empty((n * r, 7, 7, int(maps[0].shape[3])), dtype=torch.float32, device=self.device)
        props = []
        for a, b in runs:
            p, _, count = self.proposals(head if whole else [h[a:b] for h in head], image_sizes[a], padded_size)
            self.roi_align(maps if whole else [m[a:b] for m in maps], p, count, image_sizes[a], out=pooled[a * r:b * r])
            props.append((p, count))
        cls, reg = self.box_heads(pooled)
        return [((a, b), self.detections(cls[a * r:b * r], reg[a * r:b * r], p, count, image_sizes[a], original_sizes[a]))
                for (a, b), (p, count) in zip(runs, props)]


class ResNet50FPNBackbone:
    """model.backbone of fasterrcnn_resnet50_fpn (BackboneWithFPN): NHWC fp32 in, five 256-channel maps out."""

    def __init__(self, state_dict: Dict[str, np.ndarray], device="cuda:0", bn_eps: float = 0.0):
        sd, dev = state_dict, device
        b = "backbone.body."
        mk = lambda *a, **k: _Conv(sd, *a, bn_eps=bn_eps, device=dev, **k)
        self.stem = mk(b + "conv1.weight", bn=b + "bn1", stride=2, pad=3)
        self.blocks: List[List[Tuple]] = []
        for li, nblocks in enumerate(_LAYERS, start=1):
            layer = []
            for blk in range(nblocks):
                p = f"{b}layer{li}.{blk}"
                stride = 2 if (blk == 0 and li > 1) else 1
                c1 = mk(p + ".conv1.weight", bn=p + ".bn1")
                c2 = mk(p + ".conv2.weight", bn=p + ".bn2", stride=stride, pad=1)     # stride on the 3x3 ("v1.5")
                c3 = mk(p + ".conv3.weight", bn=p + ".bn3")
                ds = mk(p + ".downsample.0.weight", bn=p + ".downsample.1", stride=stride) if blk == 0 else None
                layer.append((c1, c2, c3, ds if ds is None else _DualConv(c3, ds)))
            self.blocks.append(layer)
        f = "backbone.fpn."
        self.inner = [mk(f + f"inner_blocks.{i}.weight", bias=f + f"inner_blocks.{i}.bias") for i in range(4)]
        self.outer = [mk(f + f"layer_blocks.{i}.weight", bias=f + f"layer_blocks.{i}.bias", pad=1) for i in range(4)]
        self.device = torch.device(device)

    def forward_nhwc(self, x: torch.Tensor) -> "OrderedDict[str, torch.Tensor]":
        lib = _lib.load()
        st = _stream(x.device)
        x = self.stem(x, relu=True)
        n, h, w, c = x.shape
        y = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), dtype=torch.float32, device=x.device)
        _lib.check(lib.opdet_maxpool3x3s2_f32(x.data_ptr(), y.data_ptr(), n, h, w, c, st), "opdet_maxpool3x3s2_f32")
        x = y
        feats = []
        for layer in self.blocks:
            for c1, c2, c3, ds in layer:
                out = c2(c1(x, relu=True), relu=True)
                # relu(bn3(conv3) + identity) in the epilogue; a stage's first block: conv3 and the downsample branch as one product
                x = c3(out, relu=True, residual=x) if ds is None else ds(out, x)
            feats.append(x)
        last = self.inner[3](feats[3], relu=False)
        results = [self.outer[3](last, relu=False)]
        for i in (2, 1, 0):
            # lateral conv + nearest-upsampled coarser level, added in the conv's epilogue (FeaturePyramidNetwork.forward)
            last = self.inner[i].plus_upsampled(feats[i], last)
            results.insert(0, self.outer[i](last, relu=False))
        top = results[-1]
        n, h, w, c = top.shape
        pool = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), dtype=torch.float32, device=top.device)
        _lib.check(lib.opdet_subsample2_f32(top.data_ptr(), pool.data_ptr(), n, h, w, c, st), "opdet_subsample2_f32")
        results.append(pool)
        return OrderedDict(zip(["0", "1", "2", "3", "pool"], results))


def resized_size(h: int, w: int, min_size: int = 800, max_size: int = 1333) -> Tuple[int, int]:
    """GeneralizedRCNNTransform.resize: the size F.interpolate(scale_factor=...) produces"""
    scale = min(float(min_size) / min(h, w), float(max_size) / max(h, w))
    return int(np.floor(h * scale)), int(np.floor(w * scale))


def preprocess_frame(frame_bgr: np.ndarray, device="cuda:0", min_size: int = 800, max_size: int = 1333) -> torch.Tensor:
    """uint8 [H,W,3] BGR frame (cv2 order, detector.py:71) -> NHWC fp32 [1,PH,PW,4] on the device."""
    if frame_bgr.dtype != np.uint8 or frame_bgr.ndim != 3 or frame_bgr.shape[2] != 3:
        raise ValueError("frame must be uint8 [H, W, 3] (BGR)")
    lib = _lib.load()
    h, w = frame_bgr.shape[:2]
    scale = min(float(min_size) / min(h, w), float(max_size) / max(h, w))
    rh, rw = int(np.floor(h * scale)), int(np.floor(w * scale))
    ph, pw = (rh + 31) // 32 * 32, (rw + 31) // 32 * 32
    dev = torch.device(device)
    fr = torch.from_numpy(np.ascontiguousarray(frame_bgr)).to(dev)
    y = torch.empty((1, ph, pw, 4), dtype=torch.float32, device=dev)
    mean = (ctypes.c_float * 3)(*IMAGENET_MEAN)
    std = (ctypes.c_float * 3)(*IMAGENET_STD)
    with torch.cuda.device(dev):
        rc = lib.opdet_preprocess_frame_f32(fr.data_ptr(), y.data_ptr(), h, w, rh, rw, ph, pw, mean, std, _stream(dev))
    _lib.check(rc, "opdet_preprocess_frame_f32")
    return y


class CaterObjectDetector(object):
    """reference baselines/detector.py:11-86."""

    @staticmethod
    def remove_low_probability_object(model_output: dict, accuracy_threshold: float = 0.8) -> dict:
        """detector.py:14-28: keep the first k rows, k = count(scores >= threshold) - relies on the
        detector returning scores in descending order."""
        scores = model_output["scores"]
        k = int(torch.sum((scores >= accuracy_threshold)).item())
        return {"boxes": model_output["boxes"][:k, :], "labels": model_output["labels"][:k], "scores": scores[:k]}

    def __init__(self, saved_detector_path, class_names_to_indices: dict = None, min_size: int = 800,
                 max_size: int = 1333):
        self.saved_detector_path = saved_detector_path
        self.num_classes = 193
        self.indices_to_names = {i: n for n, i in (class_names_to_indices or {}).items()}
        self.min_size, self.max_size = min_size, max_size          # fasterrcnn_resnet50_fpn defaults
        self.backbone: ResNet50FPNBackbone = None
        self.heads: FasterRCNNHeads = None

    def load_model(self, compute_device: torch.device) -> None:
        saved = torch.load(self.saved_detector_path, map_location="cpu")          # detector.py:61-63
        self.load_state_dict(saved["model_state_dict"], compute_device)

    def load_state_dict(self, state_dict, compute_device) -> None:
        self.backbone = ResNet50FPNBackbone(state_dict, device=compute_device)
        self.heads = FasterRCNNHeads(state_dict, device=compute_device, num_classes=self.num_classes)

    def backbone_features(self, frame: np.ndarray, compute_device: torch.device) -> "OrderedDict[str, torch.Tensor]":
        x = preprocess_frame(frame, compute_device, self.min_size, self.max_size)
        with torch.cuda.device(x.device):
            return self.backbone.forward_nhwc(x)

    def backbone_features_batch(self, frames, compute_device: torch.device) -> "OrderedDict[str, torch.Tensor]":
        """Several frames of a clip in ONE backbone pass ([n,240,320,3] uint8): the reference runs the detector on
        one frame per call (detector.py:80, preprocess_perception_main.py:28-41); the deep 25x34 / 50x68 maps of a
        single frame cannot fill 256 CUs, 16 frames per pass reach ~0.43 of the fp32 MFMA peak."""
        x = torch.cat([preprocess_frame(f, compute_device, self.min_size, self.max_size) for f in frames], dim=0)
        with torch.cuda.device(x.device):
            return self.backbone.forward_nhwc(x)

    MAX_FRAMES_PER_PASS = 32      # keeps every activation under the 2 GiB the conv kernel's 32-bit offsets address

    def _enqueue(self, frames, compute_device):
        """everything of one pass enqueued on the current stream; no host sync"""
        return self._enqueue_with(frames, compute_device, "forward_images")

    def _enqueue_padded(self, frames, compute_device):
        """one pass (<= MAX_FRAMES_PER_PASS frames of one shape) enqueued on the current stream, its detections left on the
        device as the batched padded tensors RoIHeads' stage writes: (boxes [p, md, 4] fp32 pixels, scores [p, md] descending,
        labels [p, md] int64, n_det [p] int32; rows >= n_det zero).  No host sync (DetectorStreams)."""
        if len(frames) > self.MAX_FRAMES_PER_PASS:
            raise ValueError(f"at most {self.MAX_FRAMES_PER_PASS} frames per pass")
        runs = self._enqueue_with(frames, compute_device, "forward_runs")
        assert len(runs) == 1, "frames of one shape are one run"
        return runs[0][1]

    def _enqueue_with(self, frames, compute_device, heads_forward: str):
        if self.backbone is None:
            raise RuntimeError("load_model() first")
        if len({f.shape for f in frames}) != 1:
            raise ValueError("frames of one call must share a shape")
        x = torch.cat([preprocess_frame(f, compute_device, self.min_size, self.max_size) for f in frames], dim=0)
        hw = [tuple(f.shape[:2]) for f in frames]
        sizes = [resized_size(h, w, self.min_size, self.max_size) for h, w in hw]
        with torch.cuda.device(x.device):
            feats = self.backbone.forward_nhwc(x)
            return getattr(self.heads, heads_forward)(feats, sizes, x.shape[1:3], hw)

    def _finish(self, outs):
        counts = torch.cat([o[3] for o in outs]).tolist()              # the one host sync of a pass
        return [self._to_dict(o[0], o[1], o[2], int(n)) for o, n in zip(outs, counts)]

    def _detect(self, frames, compute_device):
        if len(frames) > self.MAX_FRAMES_PER_PASS:
            out = []
            for i in range(0, len(frames), self.MAX_FRAMES_PER_PASS):
                out.extend(self._detect(frames[i:i + self.MAX_FRAMES_PER_PASS], compute_device))
            return out
        return self._finish(self._enqueue(frames, compute_device))

    def detect_batch_async(self, frames, compute_device):
        """enqueue one pass (<= MAX_FRAMES_PER_PASS frames) on the CURRENT stream and return a handle; `handle()` waits
        for that pass only and returns the detections.  Two passes in flight on two streams let the small per-image
        selection kernels of one pass run in the shadow of the other pass's conv GEMMs (preprocess_perception_main)."""
        if len(frames) > self.MAX_FRAMES_PER_PASS:
            raise ValueError(f"at most {self.MAX_FRAMES_PER_PASS} frames per pass")
        stream = torch.cuda.current_stream(torch.device(compute_device))
        outs = self._enqueue(list(frames), compute_device)

        def result():
            with torch.cuda.stream(stream):
                return self._finish(outs)
        return result

    @staticmethod
    def _to_dict(boxes, scores, labels, n: int) -> Dict[str, torch.Tensor]:
        return {"boxes": boxes[:n], "labels": labels[:n], "scores": scores[:n]}

    def __call__(self, frame: np.ndarray, compute_device: torch.device) -> List[Dict[str, torch.Tensor]]:
        """detector.py:71-86: BGR uint8 frame -> [{"boxes" [n,4] xyxy px, "labels" [n] int64, "scores" [n] desc}]"""
        return self._detect([frame], compute_device)

    def detect_batch(self, frames, compute_device: torch.device) -> List[Dict[str, torch.Tensor]]:
        """several frames of a clip in ONE pass: every stage, dense or selection, is one launch over the frames of the pass (DESIGN.md
        section 11); one host sync at the end.  Same results as frame by frame
        (the reference calls the detector on one frame at a time, preprocess_perception_main.py:28-41)."""
        return self._detect(list(frames), compute_device)

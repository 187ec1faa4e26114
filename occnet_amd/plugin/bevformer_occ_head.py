"""BEVFormerOccHead — owner of the BEV queries and positional encoding, thin caller of TransformerOcc.

Mirror of the reference's projects/mmdet3d_plugin/bevformer/dense_heads/bevformer_occ_head.py
(registry name, constructor kwargs — swallowing in_channels / sync_cls_avg_factor / train_cfg /
test_cfg through **kwargs and reading kwargs['num_classes'] —, `bev_embedding`,
`positional_encoding`, `transformer` attribute names, forward / loss / get_occ contracts).
"""
import os

import torch
import torch.nn as nn

from .. import derived
from .._lib import OccAmdUnsupported
from .bricks import BaseModule, CrossEntropyLoss, L1Loss
from .registry import HEADS, build_loss, build_positional_encoding, build_transformer


@HEADS.register_module()
class BEVFormerOccHead(BaseModule):

    # training: heads + both losses as ONE autograd node (ext.OccHeadsLossFunction, csrc/occ_heads_loss.hip) instead of the
    # two Sequential heads, F.cross_entropy and the elementwise L1 on materialised logits; opt-in (OCC_TRAIN_FUSED_LOSS=1)
    fused_loss = os.environ.get("OCC_TRAIN_FUSED_LOSS", "0") == "1"

    def __init__(self, *args, with_box_refine=False, as_two_stage=False, transformer=None,
                 bbox_coder=None, num_cls_fcs=2, code_weights=None,
                 pc_range=[-40, -40, -1.0, 40, 40, 5.4], bev_h=30, bev_w=30, loss_occ=None,
                 loss_flow=None, use_mask=False, positional_encoding=None, loss_depth=None, **kwargs):
        super().__init__()
        self.bev_h = bev_h
        self.bev_w = bev_w
        self.fp16_enabled = False
        self.num_classes = kwargs['num_classes']
        self.use_mask = use_mask
        self.with_box_refine = with_box_refine
        self.as_two_stage = as_two_stage
        if self.as_two_stage:
            transformer['as_two_stage'] = self.as_two_stage
        self.pc_range = pc_range
        self.real_w = self.pc_range[3] - self.pc_range[0]
        self.real_h = self.pc_range[4] - self.pc_range[1]
        self.num_cls_fcs = num_cls_fcs - 1
        self.loss_occ = build_loss(loss_occ)
        self.loss_flow = build_loss(loss_flow)
        # opt-in ray-depth supervision (ray_depth_loss.RayDepthLoss); None: no module, no code path and no number changes.
        # The geometry the config leaves out is the head's own: its pc_range, cubic voxels of real_w / bev_w, last class free.
        self.loss_depth = None
        if loss_depth is not None:
            cfg = dict(loss_depth)
            cfg.setdefault('pc_range', pc_range)
            cfg.setdefault('voxel_size', self.real_w / self.bev_w)
            cfg.setdefault('free_id', self.num_classes - 1)
            self.loss_depth = build_loss(cfg)
        self.positional_encoding = build_positional_encoding(positional_encoding)
        self.transformer = build_transformer(transformer)
        self.embed_dims = self.transformer.embed_dims
        if not self.as_two_stage:
            self.bev_embedding = nn.Embedding(self.bev_h * self.bev_w, self.embed_dims)

    def init_weights(self):
        self.transformer.init_weights()

    def _bev_pos(self, bs, device, dtype):
        """Learned positional encoding of the BEV plane, (bs, C, bev_h, bev_w).  It depends only on the two
        embedding tables, so without autograd the SAME tensor is handed out until they change: downstream
        caches (the encoder's query-major copy, the TSA position term) key on its identity."""
        pe = self.positional_encoding
        def build():
            bev_mask = torch.zeros((bs, self.bev_h, self.bev_w), device=device).to(dtype)
            return pe(bev_mask).to(dtype)
        if torch.is_grad_enabled() and any(p.requires_grad for p in pe.parameters()):
            return build()
        return derived.owned(self, '_pos').get(list(pe.parameters()), lambda: build().detach(), (bs, device, dtype))

    def _bev_inputs(self, mlvl_feats):
        """-> (bev_queries, bev_pos, grid_length) of a forward pass over mlvl_feats."""
        bs = mlvl_feats[0].shape[0]
        # the reference takes the feature dtype (bevformer_occ_head.py:118); the MI355X hot path always
        # computes in fp32 (a half-precision backbone's maps are widened when they are flattened)
        dtype = mlvl_feats[0].dtype if mlvl_feats[0].dtype == torch.float64 else torch.float32
        bev_queries = self.bev_embedding.weight.to(dtype)
        bev_pos = self._bev_pos(bs, bev_queries.device, dtype)
        return bev_queries, bev_pos, (self.real_h / self.bev_h, self.real_w / self.bev_w)

    def forward(self, mlvl_feats, img_metas, prev_bev=None, only_bev=False, test=False):
        """mlvl_feats: list of (B, N, C, H, W) -> {'bev_embed','occ','flow'}; with only_bev the
        (bs, H*W, C) BEV embedding alone (history frames)."""
        bev_queries, bev_pos, grid_length = self._bev_inputs(mlvl_feats)
        if only_bev:
            return self.transformer.get_bev_features(
                mlvl_feats, bev_queries, self.bev_h, self.bev_w, grid_length=grid_length,
                bev_pos=bev_pos, img_metas=img_metas, prev_bev=prev_bev)
        bev_embed, occ_outs, flow_outs = self.transformer(
            mlvl_feats, bev_queries, None, self.bev_h, self.bev_w, grid_length=grid_length,
            bev_pos=bev_pos, reg_branches=None, cls_branches=None, img_metas=img_metas,
            prev_bev=prev_bev)
        preds = {'bev_embed': bev_embed, 'occ': occ_outs, 'flow': flow_outs}
        cls = getattr(occ_outs, '_occ_cls', None)
        if cls is not None:     # the fused heads kernel decoded the classes in the same pass: an explicit entry
            preds['occ_cls'] = cls
        return preds

    def loss(self, voxel_semantics, voxel_flow, mask_camera, preds_dicts, gt_bboxes_ignore=None,
             img_metas=None, lidar_origins=None):
        """lidar_origins (B, T, 3), ego metres: the origins of the rays of a configured `loss_depth` (required then)."""
        loss_occ, loss_flow = self.loss_single(voxel_semantics, voxel_flow, mask_camera,
                                               preds_dicts['occ'].float(),
                                               preds_dicts['flow'].float())
        losses = dict(loss_occ=loss_occ, loss_flow=loss_flow)
        if self.loss_depth is not None:
            if lidar_origins is None:
                raise ValueError('BEVFormerOccHead.loss: loss_depth is configured and needs lidar_origins (B, T, 3)')
            targets = self.loss_depth.targets_from_occupancy(voxel_semantics, lidar_origins)
            losses['loss_depth'] = self.loss_depth(preds_dicts['occ'].float(), *targets)
        return losses

    def _fused_loss_ok(self, mlvl_feats):
        """Everything the fused heads + loss node needs that is known BEFORE the decoder runs (its BatchNorms update their
        statistics: no second pass after that): autograd on, device fp32 features, the heads and the two losses in the forms
        the kernels compute, num_classes <= 30 — and no `loss_depth`: the fused node never materialises the logits that
        the ray-depth loss renders."""
        t, lo, lf = self.transformer, self.loss_occ, self.loss_flow
        return (self.fused_loss and self.loss_depth is None and torch.is_grad_enabled() and mlvl_feats[0].is_cuda
                and mlvl_feats[0].dtype != torch.float64 and t._heads_fusable()
                and t.out_dim == 32 and t.predicter[0].weight.dtype == torch.float32
                and type(lo) is CrossEntropyLoss and type(lf) is L1Loss and lo.reduction in ('mean', 'sum')
                and lf.reduction == lo.reduction and self.num_classes <= 30)

    def forward_loss(self, mlvl_feats, img_metas, prev_bev, voxel_semantics, voxel_flow, mask_camera, lidar_origins=None):
        """loss(forward(...)) -> {'loss_occ', 'loss_flow'}; with `fused_loss` (and its conditions, _fused_loss_ok) the heads
        and both losses run as one node on the decoder features, and the logits are never materialised.  Otherwise, or when
        the node refuses its inputs, today's modules run and give today's numbers."""
        if not self._fused_loss_ok(mlvl_feats):
            return self.loss(voxel_semantics, voxel_flow, mask_camera, self(mlvl_feats, img_metas, prev_bev),
                             lidar_origins=lidar_origins)
        from .. import ext
        bev_queries, bev_pos, grid_length = self._bev_inputs(mlvl_feats)
        t = self.transformer
        _, feats = t.decoder_features(mlvl_feats, bev_queries, self.bev_h, self.bev_w, grid_length=grid_length,
                                      bev_pos=bev_pos, img_metas=img_metas, prev_bev=prev_bev)
        p, f, lo, lf = t.predicter, t.flow_predicter, self.loss_occ, self.loss_flow
        try:
            labels = voxel_semantics if voxel_semantics.dtype in (torch.uint8, torch.int64) else voxel_semantics.long()
            cw = None if lo.class_weight is None else feats.new_tensor(lo.class_weight)       # as bricks.CrossEntropyLoss
            loss_occ, loss_flow = ext.heads_loss(
                feats.contiguous(), p[0].weight, p[0].bias, p[2].weight, p[2].bias, f[0].weight, f[0].bias, f[2].weight,
                f[2].bias, labels.contiguous(), voxel_flow.contiguous(),
                mask_camera.reshape(-1).contiguous() if self.use_mask else None, cw, lo.ignore_index, lo.reduction)
        except OccAmdUnsupported:
            # the decoder has run (once): the modules take over from its features
            flow, occ = f(feats), p(feats)
            return self.loss(voxel_semantics, voxel_flow, mask_camera, {'occ': occ, 'flow': flow})
        return dict(loss_occ=lo.loss_weight * loss_occ, loss_flow=lf.loss_weight * loss_flow)

    def loss_single(self, voxel_semantics, voxel_flow, mask_camera, occ, flow):
        voxel_semantics = voxel_semantics.long()
        if self.use_mask:
            # the reference's masked branch only produces loss_occ (loss_flow is left undefined
            # there, bevformer_occ_head.py:183-188); the flow term here follows the unmasked branch
            mask_camera = mask_camera.reshape(-1)
            loss_occ = self.loss_occ(occ.reshape(-1, self.num_classes), voxel_semantics.reshape(-1),
                                     mask_camera, avg_factor=mask_camera.sum())
        else:
            loss_occ = self.loss_occ(occ.reshape(-1, self.num_classes), voxel_semantics.reshape(-1))
        loss_flow = self.loss_flow(flow.reshape(-1, 2), voxel_flow.reshape(-1, 2))
        return loss_occ, loss_flow

    def get_occ(self, preds_dicts, img_metas=None, rescale=False):
        """-> (class index per voxel (B, W, H, Z) int64, flow (B, W, H, Z, 2))."""
        occ = preds_dicts['occ']
        # 'occ_cls' (argmax of the logits, first index on ties, 0 for a row with a NaN — what softmax(-1).argmax(-1)
        # yields) is written by the fused heads kernel in the pass that writes `occ`; it is only valid while `occ` is
        # unmodified: callers that edit the logits must drop the key
        cls = preds_dicts.get('occ_cls')
        if cls is not None and cls.shape == occ.shape[:-1] and cls.device == occ.device:
            return cls, preds_dicts['flow']
        occ_score = occ.float().softmax(-1).argmax(-1)
        return occ_score, preds_dicts['flow']

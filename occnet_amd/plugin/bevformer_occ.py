"""BEVFormerOcc detector shell: images -> ResNet/FPN features (B, N, C, H, W) -> BEVFormerOccHead.

Mirror of the reference's projects/mmdet3d_plugin/bevformer/detectors/bevformer_occ.py (registry
name, constructor kwargs of the MVXTwoStageDetector call shape, `img_backbone` / `img_neck` /
`pts_bbox_head` attribute names, forward(return_loss=...) / forward_train / forward_test /
simple_test / obtain_history_bev contracts).  As in mmdet3d's MVXTwoStageDetector, the `pts` part of
train_cfg / test_cfg is injected into the head's config.
"""
import torch

from .. import cache_epoch, derived, ext
from ..io import identity_photometric, scaled_size
from .bricks import BaseModule
from .grid_mask import GridMask
from .registry import DETECTORS, build_backbone, build_head, build_neck


@DETECTORS.register_module()
class BEVFormerOcc(BaseModule):

    def __init__(self, use_grid_mask=False, pts_voxel_layer=None, pts_voxel_encoder=None,
                 pts_middle_encoder=None, pts_fusion_layer=None, img_backbone=None,
                 pts_backbone=None, img_neck=None, pts_neck=None, pts_bbox_head=None,
                 img_roi_head=None, img_rpn_head=None, train_cfg=None, test_cfg=None,
                 pretrained=None, video_test_mode=False):
        super().__init__()
        for name, v in (('pts_voxel_layer', pts_voxel_layer), ('pts_voxel_encoder', pts_voxel_encoder),
                        ('pts_middle_encoder', pts_middle_encoder), ('pts_fusion_layer', pts_fusion_layer),
                        ('pts_backbone', pts_backbone), ('pts_neck', pts_neck),
                        ('img_roi_head', img_roi_head), ('img_rpn_head', img_rpn_head)):
            if v is not None:
                raise NotImplementedError(f'{name}: the occupancy model is camera-only')
        if pts_bbox_head:
            pts_bbox_head = dict(pts_bbox_head)
            pts_bbox_head.update(train_cfg=train_cfg.get('pts') if train_cfg else None)
            pts_bbox_head.update(test_cfg=test_cfg.get('pts') if test_cfg else None)
            self.pts_bbox_head = build_head(pts_bbox_head)
        if img_backbone:
            self.img_backbone = build_backbone(img_backbone)
        if img_neck is not None:
            self.img_neck = build_neck(img_neck)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        # train-time image augmentation, applied in extract_img_feat when use_grid_mask (reference :52-53,81-82)
        self.grid_mask = GridMask(True, True, rotate=1, offset=False, ratio=0.5, mode=1, prob=0.7)
        self.use_grid_mask = use_grid_mask
        self.fp16_enabled = False
        # mixed-precision knob of THIS implementation (the reference is fp32 throughout): when set (e.g.
        # torch.bfloat16) the stock ResNet/FPN modules of the training / autograd path run under torch.autocast
        # and the FPN maps are handed to the fp32 hot path as float32.  It lives inside the detector so that
        # a DDP-wrapped model is driven through DDP.forward (the reducer must see the forward).
        self.backbone_autocast_dtype = None
        self.pretrained = pretrained
        self.video_test_mode = video_test_mode
        self.prev_frame_info = {'prev_bev': None, 'scene_token': None, 'prev_pos': 0, 'prev_angle': 0}
        self._camera_visibility = None      # visibility.CameraVisibility of a use_mask head, made at the first need (camera_visibility)

    def train(self, mode=True):
        """Mode switch + cache safety net.  Every derived-weight cache (packed Linear / chain weights, folded backbone
        plan, decoder / heads packs) is keyed on (address, _version) of its sources; writes through `.data`
        (param.data.copy_: mmcv's EMAHook swap before validation, manual loads) do not bump _version.  On a REAL
        train -> eval transition the contents are therefore fingerprinted (per tensor: 2-norm and a position-weighted sum,
        compared element by element; one host sync) and the cache epoch is bumped when they changed since the last check
        (the first check counts as a change); the eval <-> train flips inside obtain_history_bev (twice per training step)
        skip it.  NOT covered: a `.data` write while the model already is in eval mode (no transition
        to hang the check on) — call occnet_amd.invalidate_caches() after such a write."""
        was_training = self.training
        # parameters / BatchNorm statistics may change while training, and an eval() entry is where stale plans would be
        # served from: re-check the folded plan's sources at the next forward in either case
        object.__setattr__(self, '_plan_dirty', True)
        out = super().train(mode)
        if was_training and not mode and not getattr(self, '_in_history', False):
            fp = self._content_fingerprint()
            old = getattr(self, '_content_fp', None)
            if fp is not None and (old is None or old.shape != fp.shape or not torch.equal(old, fp)):
                from .bricks import _bump_cache_epoch
                _bump_cache_epoch()
                object.__setattr__(self, '_content_fp', fp)
        return out

    def _content_fingerprint(self):
        """(n_tensors, 2) float64 host tensor — per device parameter / buffer its 2-norm and its sum weighted by a fixed
        pseudo-random ramp over the element index (None on the host or without floating-point tensors): changes whenever a
        weight is rewritten, however it was written.  The weighted sum is ORDER-sensitive: a sign flip, a permutation or two
        equal-norm tensors trading places, which a sum of norms cannot see, all move it."""
        ts = [t.detach() for t in list(self.parameters()) + list(self.buffers()) if t.is_cuda and t.is_floating_point()]
        if not ts:
            return None
        n_max = max(t.numel() for t in ts)
        ramp = getattr(self, '_fp_ramp', None)
        if ramp is None or ramp.numel() < n_max or ramp.device != ts[0].device:
            idx = torch.arange(n_max, device=ts[0].device, dtype=torch.float32)
            ramp = torch.frac(torch.sin(idx * 12.9898 + 0.5) * 43758.5453) + 0.5           # in (-0.5, 1.5), fixed
            object.__setattr__(self, '_fp_ramp', ramp)
        norms = torch._foreach_norm(ts)
        dots = [torch.dot(t.reshape(-1).float(), ramp[:t.numel()]) for t in ts]
        return torch.stack([torch.stack([n.double() for n in norms]), torch.stack([d.double() for d in dots])], 1).cpu()

    def _backbone_signature(self):
        mods = [m for m in (getattr(self, 'img_backbone', None), getattr(self, 'img_neck', None)) if m is not None]
        return derived.signature(t for m in mods for t in list(m.parameters()) + list(m.buffers()))

    def _current_plan(self):
        """The folded inference backbone, rebuilt when its source parameters changed since the fold."""
        plan = getattr(self, '_inference_backbone', None)
        if plan is None:
            return None
        stale = plan.built_epoch != cache_epoch()
        if not stale and getattr(self, '_plan_dirty', False):
            stale = plan.signature != self._backbone_signature()
            object.__setattr__(self, '_plan_dirty', self.training)
        if stale:
            self.enable_fused_backbone(**self._inference_backbone_args)
            plan = self._inference_backbone
        return plan

    @property
    def with_img_neck(self):
        return hasattr(self, 'img_neck') and self.img_neck is not None

    def init_weights(self):
        for m in (getattr(self, 'img_backbone', None), getattr(self, 'pts_bbox_head', None)):
            if m is not None:
                m.init_weights()

    def extract_img_feat(self, img, img_metas=None, len_queue=None, grid_masked=False):
        """img (B, N, 3, H, W) -> list of (B, N, C, h, w) (or (B/len_queue, len_queue, N, C, h, w)).
        grid_masked: the caller has applied GridMask already (extract_feat_u8 with `aug`)."""
        if img is None:
            return None
        B = img.size(0)
        if img.dim() == 5:
            B, N, C, H, W = img.size()
            img = img.reshape(B * N, C, H, W)
        plan = None
        if not self.training and not torch.is_grad_enabled():
            plan = self._current_plan()     # refolded if the parameters were reloaded / trained since the fold
        if plan is not None:
            img_feats = plan(img)       # BN-folded, NHWC, own bf16 kernels
        else:
            if self.use_grid_mask and not grid_masked:
                img = self.grid_mask(img)
            ac = self.backbone_autocast_dtype
            with torch.autocast(img.device.type, dtype=ac or torch.bfloat16, enabled=ac is not None):
                img_feats = self.img_backbone(img)
                if isinstance(img_feats, dict):
                    img_feats = list(img_feats.values())
                if self.with_img_neck:
                    img_feats = self.img_neck(img_feats)
            if ac is not None:
                img_feats = [f.float() for f in img_feats]
        out = []
        for f in img_feats:
            BN, C, H, W = f.size()
            if len_queue is not None:
                out.append(f.view(int(B / len_queue), len_queue, int(BN / B), C, H, W))
            else:
                out.append(f.view(B, int(BN / B), C, H, W))
                # max|x| over the maps, accumulated by the plan's FPN output convolutions (backbone_plan.py): rides on the views
                am = ext.absmax_of(f)
                if am is not None:
                    ext.attach_absmax(out[-1], am)
        return out

    def enable_fused_backbone(self, dtype=torch.bfloat16, hip_tail=True, use_graph=False, fused_bottleneck=True,
                              fuse_next_stage=True):
        """Inference-only: run ResNet+FPN through FusedInferenceBackbone (eval BN folded into the
        convolutions, NHWC; with hip_tail on bf16 the stem, the 64-channel bottlenecks and the 1x1 / 3x3
        convolutions run on this repository's kernels with bias, residual and ReLU in their epilogues; with fuse_next_stage
        the last layer1 block also computes layer2's first conv1 and shortcut).  Call again
        after changing backbone weights; pass dtype=None to disable."""
        from .backbone import FusedInferenceBackbone
        object.__setattr__(self, '_inference_backbone', None)
        object.__setattr__(self, '_inference_backbone_args', dict(
            dtype=dtype, hip_tail=hip_tail, use_graph=use_graph, fused_bottleneck=fused_bottleneck,
            fuse_next_stage=fuse_next_stage))
        # folded while training (no explicit .train() call needed for that): the sources may move before the first forward
        object.__setattr__(self, '_plan_dirty', bool(self.training))
        if dtype is not None:
            plan = FusedInferenceBackbone(self.img_backbone, self.img_neck, dtype=dtype, hip_tail=hip_tail,
                                          fused_bottleneck=fused_bottleneck, fuse_next_stage=fuse_next_stage)
            plan.use_graph = use_graph
            plan.built_epoch = cache_epoch()
            plan.signature = self._backbone_signature()
            object.__setattr__(self, '_inference_backbone', plan)   # not a sub-module: owns copies
        return self

    def extract_feat(self, img, img_metas=None, len_queue=None):
        return self.extract_img_feat(img, img_metas, len_queue=len_queue)

    def _train_input_u8(self, frames_u8, img_norm_cfg, size_divisor, aug, img_scale=None):
        """(NI, Hs, Ws, 3) uint8 frames -> the (NI, 3, H, W) float32 backbone input in one launch
        (ext.train_input_u8): photometric distortion with the records `aug`, normalise, pad and — where
        extract_img_feat would apply the GridMask module — the module's mask from its own draws
        (GridMask.sample_params: same RNG consumption as the module's forward, which is then skipped).  A GridMask
        with rotate > 1 or offset=True has no closed form in the kernel: the module is applied to the result.
        img_scale: RandomScaleImageMultiViewImage(scales=[img_scale]) between normalise and pad (ext.input_u8_scaled);
        H x W, which the mask is drawn for, is then the padded size of the scaled image."""
        NI, Hs, Ws, _ = frames_u8.shape
        d = int(size_divisor)
        Hd, Wd = (Hs, Ws) if img_scale is None else scaled_size(Hs, Ws, img_scale)
        H, W = (Hd + d - 1) // d * d, (Wd + d - 1) // d * d
        gm, module_mask = None, False
        plan_serves = not self.training and not torch.is_grad_enabled() and self._current_plan() is not None
        if self.use_grid_mask and not plan_serves:
            g = self.grid_mask
            if g.rotate == 1 and not g.offset:
                drawn = g.sample_params(H, W)
                if drawn is not None:
                    gm = tuple(drawn) + (int(bool(g.use_h)), int(bool(g.use_w)), int(g.mode))
            else:
                module_mask = True
        norm = (img_norm_cfg['mean'], img_norm_cfg['std'], bool(img_norm_cfg.get('to_rgb', True)))
        if img_scale is None:
            x = ext.train_input_u8(frames_u8, aug, *norm, size_divisor=d, grid_mask=gm)
        else:
            x, _ = ext.input_u8_scaled(frames_u8, aug, *norm, img_scale, size_divisor=d, grid_mask=gm)
        return self.grid_mask(x) if module_mask else x

    def extract_feat_u8(self, img_u8, img_norm_cfg, size_divisor=32, aug=None, len_queue=None, img_scale=None,
                        img_metas=None):
        """Device-side input path: img_u8 (B, N, Hs, Ws, 3) uint8 HWC raw camera images on
        the device.  NormalizeMultiviewImage(**img_norm_cfg) + PadMultiViewImage(size_divisor) + the layout
        change of DefaultFormatBundle3D (reference transform_3d.py:31-45,82-94) run inside the stem kernel of
        the inference plan, or as torch device ops without it.  -> (list of (B, N, C, h, w) maps, padded (H, W)).
        aug: (B * N, 8) photometric records (io.sample_photometric / io.identity_photometric) select the training
        input kernel instead: distortion + normalise + pad + GridMask in one launch (_train_input_u8), then the
        backbone as extract_img_feat runs it.
        img_scale: the image scale of RandomScaleImageMultiViewImage; takes the same kernel route (ext.input_u8_scaled),
        with the identity records when `aug` is None.  img_metas: with a scale, the metas of these B samples, checked before
        any launch to be those of the scaled and padded images (_check_scaled_metas)."""
        B, N, Hs, Ws, _ = img_u8.shape
        if img_scale is not None and img_metas is not None:
            self._check_scaled_metas(img_metas, (Hs, Ws), img_scale, size_divisor)
        if img_scale is not None and aug is None:
            aug = identity_photometric(B * N)
        if aug is not None:
            x = self._train_input_u8(img_u8.reshape(B * N, Hs, Ws, 3), img_norm_cfg, size_divisor, aug, img_scale)
            H, W = x.shape[-2:]
            return self.extract_img_feat(x.view(B, N, 3, H, W), len_queue=len_queue, grid_masked=True), (H, W)
        mean, std = img_norm_cfg['mean'], img_norm_cfg['std']
        to_rgb = bool(img_norm_cfg.get('to_rgb', True))
        plan = None if self.training else self._current_plan()
        if plan is not None and getattr(plan, '_stem_fused', False):
            feats, hw = plan.forward_u8(img_u8.reshape(B * N, Hs, Ws, 3), mean, std, to_rgb, size_divisor)
        else:
            x = img_u8.reshape(B * N, Hs, Ws, 3).float()
            if to_rgb:
                x = x.flip(-1)
            stdinv = [float(1.0 / float(torch.tensor(v, dtype=torch.float32))) for v in std]   # mmcv: * (1 / std)
            x = (x - x.new_tensor(mean)) * x.new_tensor(stdinv)
            d = int(size_divisor)
            H, W = (Hs + d - 1) // d * d, (Ws + d - 1) // d * d
            x = torch.nn.functional.pad(x.permute(0, 3, 1, 2), (0, W - Ws, 0, H - Hs))
            return self.extract_img_feat(x.reshape(B, N, 3, H, W).contiguous()), (H, W)
        out = []
        for f in feats:
            BN, C, H, W = f.size()
            out.append(f.view(B, N, C, H, W))
            am = ext.absmax_of(f)
            if am is not None:
                ext.attach_absmax(out[-1], am)
        return out, hw

    def load_checkpoint(self, path_or_state, strict=False, map_location='cpu'):
        """Load an mmcv-format checkpoint ({'state_dict': ..., 'meta': ...}, what the reference's
        `load_checkpoint(model, ckpt, map_location='cpu')` reads, tools/test.py:213) or a bare state_dict; a
        'module.' prefix (saved from a DDP wrapper) is stripped.  Every derived-weight cache is invalidated.
        -> (missing_keys, unexpected_keys)."""
        from .. import invalidate_caches
        ckpt = path_or_state
        if isinstance(ckpt, (str, bytes)) or hasattr(ckpt, '__fspath__'):
            ckpt = torch.load(ckpt, map_location=map_location, weights_only=False)
        sd = ckpt.get('state_dict', ckpt) if isinstance(ckpt, dict) else ckpt
        sd = {(k[7:] if k.startswith('module.') else k): v for k, v in sd.items()}
        res = self.load_state_dict(sd, strict=strict)
        invalidate_caches(self)
        return list(res.missing_keys), list(res.unexpected_keys)

    def forward_pts_train(self, pts_feats, gt_bboxes_3d, gt_labels_3d, voxel_semantics, voxel_flow,
                          mask_camera, img_metas, gt_bboxes_ignore=None, prev_bev=None, lidar_origins=None):
        depth = {} if lidar_origins is None else dict(lidar_origins=lidar_origins)      # a head's configured loss_depth
        if getattr(self.pts_bbox_head, 'fused_loss', False):     # heads + losses as one node (OCC_TRAIN_FUSED_LOSS)
            return self.pts_bbox_head.forward_loss(pts_feats, img_metas, prev_bev, voxel_semantics, voxel_flow, mask_camera,
                                                   **depth)
        outs = self.pts_bbox_head(pts_feats, img_metas, prev_bev)
        return self.pts_bbox_head.loss(voxel_semantics, voxel_flow, mask_camera, outs,
                                       img_metas=img_metas, **depth)

    def forward(self, return_loss=True, **kwargs):
        if return_loss:
            return self.forward_train(**kwargs)
        return self.forward_test(**kwargs)

    def obtain_history_bev(self, imgs_queue, img_metas_list, img_norm_cfg=None, img_aug=None, img_scale=None):
        """BEV of the history frames, iteratively, without gradients
        (imgs_queue (bs, len_queue, N, 3, H, W), or raw uint8 frames (bs, len_queue, N, Hs, Ws, 3) with
        img_norm_cfg, optional (bs * len_queue * N, 8) photometric records img_aug and an optional img_scale, as forward_train
        takes them)."""
        was_training = self.training
        object.__setattr__(self, '_in_history', True)      # no content fingerprint for this eval <-> train flip
        self.eval()
        object.__setattr__(self, '_in_history', False)
        with torch.no_grad():
            prev_bev = None
            if imgs_queue.dtype == torch.uint8:
                bs, len_queue, num_cams, Hs, Ws, _ = imgs_queue.shape
                if img_aug is None:
                    img_aug = identity_photometric(bs * len_queue * num_cams)
                img_feats_list, _ = self.extract_feat_u8(imgs_queue.reshape(bs * len_queue, num_cams, Hs, Ws, 3),
                                                         img_norm_cfg, aug=img_aug, len_queue=len_queue, img_scale=img_scale,
                                                         img_metas=[each[i] for each in img_metas_list for i in range(len_queue)])
            else:
                bs, len_queue, num_cams, C, H, W = imgs_queue.shape
                imgs_queue = imgs_queue.reshape(bs * len_queue, num_cams, C, H, W)
                img_feats_list = self.extract_feat(img=imgs_queue, len_queue=len_queue)
            for i in range(len_queue):
                img_metas = [each[i] for each in img_metas_list]
                if not img_metas[0]['prev_bev_exists']:
                    prev_bev = None
                img_feats = [each_scale[:, i] for each_scale in img_feats_list]
                prev_bev = self.pts_bbox_head(img_feats, img_metas, prev_bev, only_bev=True)
        if was_training:
            self.train()
        return prev_bev

    def camera_visibility(self, voxel_semantics):
        """The CameraVisibility that makes `mask_camera` for a use_mask head from the ground truth and img_metas alone, made at
        the first call and again when the grid or the device changes: the head's pc_range, the device the model's parameters
        are on, and the grid's voxel size — pc_range's x extent over the grid's X; the grid must have cubic voxels
        (ValueError otherwise: the ray caster has one voxel size)."""
        head = self.pts_bbox_head
        pc_range = [float(v) for v in head.pc_range]
        shape = tuple(voxel_semantics.shape[-3:])
        sizes = [(pc_range[3 + k] - pc_range[k]) / shape[k] for k in range(3)]
        if max(sizes) - min(sizes) > 1e-6 * max(sizes):
            raise ValueError(f'camera_visibility: pc_range {pc_range} over a {shape} grid has no single voxel size ({sizes})')
        device = next(self.parameters()).device
        cv = self._camera_visibility
        if cv is None or cv.device != device or tuple(cv.occ_size) != shape:
            from ..visibility import CameraVisibility
            cv = self._camera_visibility = CameraVisibility(pc_range, sizes[0], free_id=head.num_classes - 1, device=device)
        return cv

    def forward_train(self, points=None, img_metas=None, gt_bboxes_3d=None, gt_labels_3d=None,
                      voxel_semantics=None, voxel_flow=None, mask_lidar=None, mask_camera=None,
                      gt_labels=None, gt_bboxes=None, img=None, proposals=None,
                      gt_bboxes_ignore=None, img_depth=None, img_mask=None, img_u8=None, img_norm_cfg=None,
                      img_aug=None, img_scale=None, lidar_origins=None):
        """lidar_origins (B, T, 3), ego metres (io.lidar_origins): the ray origins of the head's `loss_depth`, when configured.
        img_u8 (B, N, Hs, Ws, 3) uint8 device frames + img_norm_cfg (+ img_aug, (B * N, 8) records of
        io.sample_photometric; identity when None) instead of `img`: the input tensor is built on the device by
        ext.train_input_u8, GridMask included when use_grid_mask.  img_scale: the frames are rescaled on the way
        (ext.input_u8_scaled); img_metas must be those of the scaled images (io.scale_img_metas)."""
        if img_u8 is not None:
            if img is not None:
                raise ValueError('forward_train: pass img or img_u8, not both')
            if img_aug is None:
                img_aug = identity_photometric(img_u8.shape[0] * img_u8.shape[1])
            img_feats, _ = self.extract_feat_u8(img_u8, img_norm_cfg, aug=img_aug, img_scale=img_scale, img_metas=img_metas)
        else:
            if img_scale is not None:
                raise ValueError('forward_train: img_scale rescales img_u8 frames; an `img` tensor is taken as it is')
            img_feats = self.extract_feat(img=img, img_metas=img_metas)
        if mask_camera is None and getattr(self.pts_bbox_head, 'use_mask', False):
            mask_camera = self.camera_visibility(voxel_semantics)(voxel_semantics, img_metas)
        losses = dict()
        losses.update(self.forward_pts_train(img_feats, gt_bboxes_3d, gt_labels_3d, voxel_semantics,
                                             voxel_flow, mask_camera, img_metas, gt_bboxes_ignore,
                                             prev_bev=None,
                                             **({} if lidar_origins is None else dict(lidar_origins=lidar_origins))))
        return losses

    def forward_test(self, img_metas, img=None, voxel_semantics=None, mask_lidar=None,
                     mask_camera=None, **kwargs):
        if not isinstance(img_metas, list):
            raise TypeError('img_metas must be a list, but got {}'.format(type(img_metas)))
        img = [img] if img is None else img
        new_prev_bev, occ_results, flow_results = self.simple_test(img_metas[0], img[0],
                                                                   prev_bev=None, **kwargs)
        return {'occ_results': occ_results.cpu(), 'flow_results': flow_results.cpu()}

    def simple_test_pts(self, x, img_metas, prev_bev=None, rescale=False):
        outs = self.pts_bbox_head(x, img_metas, prev_bev=prev_bev, test=True)
        occ, flow = self.pts_bbox_head.get_occ(outs, img_metas, rescale=rescale)
        return outs['bev_embed'], occ, flow

    @staticmethod
    def _check_scaled_metas(img_metas, frames_hw, img_scale, size_divisor):
        """With an image scale the caller scales the metas, as the reference's pipeline does; scaled images under unscaled
        matrices would project every reference point to the wrong pixel without any error.  Checked before any launch:
        every img_shape must be the padded size of the (Hs, Ws) = frames_hw frames at img_scale."""
        hd, wd = scaled_size(frames_hw[0], frames_hw[1], img_scale)
        d = int(size_divisor)
        hw = ((hd + d - 1) // d * d, (wd + d - 1) // d * d)
        for b, meta in enumerate(img_metas):
            for v, shape in enumerate(meta['img_shape']):
                if tuple(int(n) for n in shape[:2]) != hw:
                    raise ValueError(f"img_scale: img_metas[{b}]['img_shape'][{v}] is {tuple(shape)}, the scaled and padded "
                                     f"images are {hw}: pass metas scaled by io.scale_img_metas")

    def simple_test(self, img_metas, img=None, prev_bev=None, rescale=False, img_u8=None, img_norm_cfg=None, img_scale=None):
        """img_u8 (B, N, Hs, Ws, 3) uint8 device frames + img_norm_cfg instead of `img`: extract_feat_u8's route, the stem
        of the inference plan reading the frames where there is one.  img_scale: the frames are rescaled on the way
        (ext.input_u8_scaled -> the backbone); img_metas must be those of the scaled images (io.scale_img_metas)."""
        if img_u8 is not None:
            if img is not None:
                raise ValueError('simple_test: pass img or img_u8, not both')
            img_feats, _ = self.extract_feat_u8(img_u8, img_norm_cfg, img_scale=img_scale, img_metas=img_metas)
        else:
            if img_scale is not None:
                raise ValueError('simple_test: img_scale rescales img_u8 frames; an `img` tensor is taken as it is')
            img_feats = self.extract_feat(img=img, img_metas=img_metas)
        return self.simple_test_pts(img_feats, img_metas, prev_bev, rescale=rescale)

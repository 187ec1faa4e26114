"""numpy restatement of the submission rows for ANY grid geometry (test infrastructure for csrc/submission_rays.hip).

`rows()` is metrics.process_one_sample with the hard-coded range, voxel size and free id turned into arguments: the same tensor
statements (so the arithmetic follows the origins' float type through torch's promotion exactly as there), one call of
`ext.dvr_render_forward` per origin — the caster that tests/test_gpu_dvr.py pins to the reference's kernel bit for bit — and
numpy indexing of class and flow at the reported voxel.  `pack()` is the reference's conversion to the file's types
(nuscenes_occ.py:232-234), `cls_int8()` the rule for class ids that astype(np.int8) on a float leaves undefined."""
import numpy as np
import torch


def align256(n):
    return (int(n) + 255) // 256 * 256


def layout(B, Tmax, R):
    """(N, off_cls, off_dist, off_flow, total) of the packed buffer: int8[N] | fp16[N] | fp16[N][2], 256-byte sections."""
    n = B * Tmax * R
    return n, 0, align256(n), align256(n) + align256(2 * n), align256(n) + align256(2 * n) + align256(4 * n)


def cls_int8(ids):
    """Class ids (any integer array) -> int8 by two's-complement wrap of the low 8 bits; equals astype(np.int8) of the float
    row for ids 0..127 (the range the host path defines)."""
    return (np.asarray(ids).astype(np.int64) & 0xff).astype(np.uint8).view(np.int8)


def rows(sem, flow, origins, rays, pc_min, voxel_size, free_id=16, device='cuda'):
    """sem (X, Y, Z) integer numpy, flow (X, Y, Z, 2) float32 numpy, origins (T, 3) float32 / float64 tensor in metres, rays
    (R, 3) float32 tensor -> (labels int64 (T*R), rows float32 (T*R, 4): label, depth, flow_x, flow_y)."""
    from occnet_amd import ext
    sem = np.asarray(sem)
    flow = np.asarray(flow, dtype=np.float32)
    occ = np.where(sem == free_id, 0, 1)
    occ_pred = torch.from_numpy(occ).permute(2, 1, 0)[None, None].contiguous().float()
    offset = torch.tensor([float(v) for v in pc_min], dtype=torch.float32)[None, None, :]
    scaler = torch.tensor([float(voxel_size)] * 3, dtype=torch.float32)[None, None, :]
    tindex = torch.zeros([1, rays.shape[0]])
    output_origin = origins[None]
    labels, out = [], []
    for t in range(output_origin.shape[1]):
        lidar_origin = output_origin[:, t:t + 1, :]
        lidar_endpts = rays[None] + lidar_origin
        origin_render = ((lidar_origin - offset) / scaler).float()
        points_render = ((lidar_endpts - offset) / scaler).float()
        dist, _, coord = ext.dvr_render_forward(occ_pred.to(device), origin_render.to(device), points_render.to(device),
                                                tindex.to(device), [1] + list(occ_pred.shape[2:]), "test")
        dist = (dist * scaler[0, 0, 0].to(device)).cpu()          # float32 distance * float32 voxel size
        c = coord[0].int().cpu().numpy()
        lab = sem[c[:, 0], c[:, 1], c[:, 2]].astype(np.int64)
        f = torch.from_numpy(flow[c[:, 0], c[:, 1], c[:, 2]])
        labels.append(lab)
        out.append(torch.cat([torch.from_numpy(lab)[:, None].float(), dist[0, :, None], f.float()], -1))
    return np.concatenate(labels), torch.cat(out, 0).numpy()


def pack(labels, rows_f32):
    """-> (pcd_cls int8, pcd_dist float16, pcd_flow float16 (n, 2))"""
    return cls_int8(labels), rows_f32[:, 1].astype(np.float16), rows_f32[:, 2:4].astype(np.float16)

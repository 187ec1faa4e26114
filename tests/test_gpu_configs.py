"""-m gpu: the remaining BASELINE.json configs as parity / consistency cases.

configs[2] temporal queue (4-frame history through obtain_history_bev), configs[4] high-resolution
400x400x32 grid (full size: all fused kernels vs the library-op execution of the same model; the CPU
oracle needs minutes per layer at this size, so the oracle comparison is done on a 1/10-scale grid of the
same structure: Z = 32, 8 decoder input channels)."""
import os

import pytest
import torch

from occnet_amd import synthetic
from tests.util import TOL, build_pair, maxdiff, small_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_temporal_queue_matches_oracle_chain():
    """BEVFormerOcc.obtain_history_bev over a 4-frame queue (reference bevformer_occ.py:159-178): frame i
    attends to the rotated BEV of frame i-1; `prev_bev_exists=False` resets the chain.  Checked against
    the oracle head driven through the same chain on the same per-frame features."""
    from occnet_amd.plugin import BEVFormerOcc
    g = small_cfg(bev=(24, 24), num_layers=1)
    prod, ora = build_pair(g, seed=6)
    det = BEVFormerOcc.__new__(BEVFormerOcc)
    torch.nn.Module.__init__(det)
    det.pts_bbox_head = prod
    det.video_test_mode = True
    L = 4
    frames = [synthetic.make_features(g, seed=60 + i) for i in range(L)]
    metas_list = [[]]
    for i in range(L):
        m = synthetic.make_img_metas(g, seed=i)[0]
        m['prev_bev_exists'] = i != 2          # frame 2 starts a new scene: history dropped
        m['can_bus'][-1] = 3.0 * i             # ego yaw change since the previous frame (degrees)
        metas_list[0].append(m)
    # (bs, len_queue, ...) features per level, as extract_feat(len_queue=L) returns them
    stacked = [torch.stack([frames[i][l][0] for i in range(L)], 0)[None].cuda()
               for l in range(len(frames[0]))]
    det.extract_feat = lambda img, img_metas=None, len_queue=None: stacked
    imgs = torch.zeros(1, L, g['num_cams'], 3, 8, 8, device='cuda')
    bev_p = det.obtain_history_bev(imgs, metas_list)
    prev = None
    with torch.no_grad():
        for i in range(L):
            if not metas_list[0][i]['prev_bev_exists']:
                prev = None
            prev = ora(frames[i], [metas_list[0][i]], prev, only_bev=True)
    d = maxdiff(bev_p, prev)
    print(f"4-frame queue BEV: max|hip - oracle| = {d:.3e}")
    assert bev_p.shape == prev.shape
    assert d < TOL


def test_hires_structure_matches_oracle():
    """configs[4] structure at a size the oracle finishes in seconds: pillar_h = 32 -> 8 decoder input
    channels (Conv3d kernel <Z=32, CH=8> for the lifter, <32, 16> for the second conv)."""
    g = small_cfg(bev=(20, 24), pillar_h=32, num_layers=1)
    prod, ora = build_pair(g, seed=7)
    feats = synthetic.make_features(g, seed=7)
    metas = synthetic.make_img_metas(g)
    with torch.no_grad():
        out_o = ora(feats, metas)
        out_p = prod([f.cuda() for f in feats], metas)
    assert out_p['occ'].shape == (1, 24, 20, 32, 17)
    for k in ('bev_embed', 'occ', 'flow'):
        d = maxdiff(out_p[k], out_o[k])
        print(f"hires-structure {k}: max|hip - oracle| = {d:.3e}")
        assert d < TOL


def test_hires_full_size_fused_vs_library_ops():
    """400x400x32 (160 000 queries, 5.12 M voxels) at full size: every fused kernel vs the same model
    executed with library GEMMs / torch LayerNorm / MIOpen Conv3d (gather kernels shared)."""
    from occnet_amd.plugin import BEVFormerLayer, Config, build_head, import_plugin
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'occ_hires_400x400x32.py'))
    import_plugin(cfg)
    from tests.util import randomize
    head = build_head(cfg.model.pts_bbox_head)
    randomize(head, 5)
    head = head.cuda().eval()
    g = dict(synthetic.HIRES)
    feats = [f.cuda() for f in synthetic.make_features(g, seed=5)]
    metas = synthetic.make_img_metas(g)
    with torch.no_grad():
        a = head(feats, metas)
        a = {k: v.clone() for k, v in a.items()}
        for m in head.modules():
            if isinstance(m, BEVFormerLayer):
                m.use_fused = False
        head.transformer.use_fused_decoder = False
        b = head(feats, metas)
    assert a['occ'].shape == (1, 400, 400, 32, 17) and a['flow'].shape == (1, 400, 400, 32, 2)
    for k in ('bev_embed', 'occ', 'flow'):
        d = maxdiff(a[k], b[k])
        print(f"hires 400x400x32 {k}: fused vs library ops max diff = {d:.3e}")
        assert d < 5e-4        # the fused path gathers fp16 value rows, the library path fp32 ones


def test_bench_multi_rank_plumbing(tmp_path):
    """`bench.py` as the driver launches it for N > 1 (torch.distributed.run, one process per rank): rank
    env parsing, barrier + MAX-over-ranks timing, whole-job value = N*K/t, ONE JSON line from rank 0.  Run
    with 2 ranks sharing the single GPU of the test box (OCC_BENCH_SHARE_GPU=1 -> gloo group); the real
    multi-GPU run uses the same code path with RCCL."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, OCC_BENCH_SHARE_GPU="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29541", os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "3", "--warmup", "1", "--scope", "hotpath", "--no-cpu-baseline", "--full"]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["scaling"] == "weak"
    assert out["config"]["global_batch"] == 2 and out["config"]["parallelism"] == "dp2"
    assert abs(out["value"] - 2 * 3 / (out["ms_per_step"] * 3e-3)) / out["value"] < 1e-6
    assert "roofline" in out and "cpu_baseline" not in out


def test_bench_self_launch_two_ranks():
    """`python bench.py --gpus 2` WITHOUT torchrun (how a user, and possibly the driver, invokes it; the reference's
    tools/dist_train.sh:9-11 role): bench.py re-executes itself under torch.distributed.run on 127.0.0.1 and rank 0
    prints one JSON line with n_gpus = 2.  Both ranks share the test box's single GPU (gloo group)."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
    env.update(OCC_BENCH_SHARE_GPU="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--scope", "hotpath", "--no-cpu-baseline"]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["config"]["parallelism"] == "dp2"
    # a plain run (no --full) reports the headline only: no roofline, per-kernel or second-pass figures
    assert not {"roofline", "mfma_kernels", "value_no_instrumentation", "host_enqueue_ms_per_step"} & set(out)

"""GPU parity of the whole forward (bde2vid_amd.model.BDE2VID through bde_forward) against the
golden frames of the reference.  Tolerance: north_star's 1e-3 max-abs on the sigmoid output is the
contract; the assertion is 2e-4 (fp32 MFMA accumulation order + folded LayerNorm only)."""
import numpy as np
import pytest
import torch

from tests.util import (load_golden, case_from_meta, maxabs, E2E_CASES, CFGA_SAMPLED, LONGT_CASES, VARIANT_CASES,
                        assert_sampled)

pytestmark = pytest.mark.gpu
TOL = 2e-4


def run_case(meta):
    from bde2vid_amd.model import build_model
    cfg, sd, xs = case_from_meta(meta)
    m = build_model(cfg, sd, 'cuda:0')
    with torch.no_grad():
        ys = m([{'events': torch.from_numpy(x).cuda()} for x in xs])
    return m, cfg, sd, xs, torch.stack(ys)


@pytest.mark.parametrize('name', sorted(E2E_CASES))
def test_e2e_matches_reference(name):
    z, meta = load_golden(name)
    m, cfg, sd, xs, y = run_case(meta)
    assert tuple(y.shape) == z['out'].shape
    assert maxabs(y, z['out']) <= TOL


@pytest.mark.parametrize('name', sorted(VARIANT_CASES))
def test_constructor_variants_match_reference(name):
    """Every constructor flag of the reference generator besides the assumed canonical ones (V5.py:19-23): ConvGRU, bare
    ConvLayer encoders (useRC=False), skip_concat with its 1x1 fusion convs, the ResidualBlockNoBN bottleneck on buffer slot 0
    (depths[-1] == 0; buffer_index[0] negative and positive), BatchNorm / InstanceNorm in eval mode, and all of them at once --
    against whole forwards of the real reference.  The configuration is also recovered from the state dict alone."""
    from bde2vid_amd.model import BDE2VID
    from bde2vid_amd.weights import infer_config
    z, meta = load_golden(name)
    m, cfg, sd, xs, y = run_case(meta)
    assert tuple(y.shape) == z['out'].shape
    assert maxabs(y, z['out']) <= TOL
    inferred = infer_config(sd, buffer_index=cfg.buffer_index, q_idx=cfg.q_idx)
    for k in ('recurrent_block_type', 'useRC', 'skip_type', 'norm_kind', 'depths', 'basechannels', 'ks', 'num_heads'):
        assert getattr(inferred, k) == getattr(cfg, k), k
    if cfg.bottleneck:
        assert inferred.num_res_blocks == cfg.num_res_blocks
    # the receiver side of the weight broadcast allocates the same packed layout for every variant
    b = BDE2VID(generator=cfg).to('cuda:0').alloc_packed()
    assert b.packed_view().shape == m.packed_view().shape


def test_e2e_config_a_full_size():
    z, meta = load_golden('e2e_cfgA_184x240')
    m, cfg, sd, xs, y = run_case(meta)
    s = meta['stride']
    assert maxabs(y[..., ::s, ::s], z['out']) <= TOL
    assert np.allclose(y.mean(dim=(1, 2, 3, 4)).cpu().numpy(), z['mean'], atol=1e-5)


def test_intermediates_match_oracle():
    """Stage-by-stage against the oracle's captured intermediates (pre-sigmoid, O(1) magnitudes)."""
    from oracle import bde2vid_oracle as O
    z, meta = load_golden('e2e_tiny')
    m, cfg, sd, xs, y = run_case(meta)
    cap = {}
    with torch.no_grad():
        O.forward(sd, cfg, [{'events': torch.from_numpy(x)} for x in xs], capture=cap)
    T, B = meta['T'], meta['B']
    head = m.get_intermediate('head', cap['head'].shape)
    assert maxabs(head, cap['head']) <= 1e-4
    for l in range(cfg.num_encoders):
        ref = cap.get(f'refined{l}', cap[f'merged{l}'])
        got = m.get_intermediate(f'merged{l}', ref.shape)
        assert maxabs(got, ref) <= 5e-4, f'level {l}'


def test_forward_is_stateless_and_repeatable():
    z, meta = load_golden('e2e_T2')
    m, cfg, sd, xs, y1 = run_case(meta)
    inp = [{'events': torch.from_numpy(x).cuda()} for x in xs]
    y2 = torch.stack(m(inp))
    y3 = torch.stack(m(inp))
    assert torch.equal(y2, y3)           # zero state at every call (bde2vid.py:31), deterministic kernels
    assert maxabs(y1, y2) == 0.0


def test_chunk_independence_property():
    """Size-independent property at a BASELINE size: a sequence's frames do not depend on batch
    neighbours -- batch of two different sequences == the two sequences run alone."""
    from bde2vid_amd.model import build_model
    from bde2vid_amd.config import GeneratorConfig
    from bde2vid_amd.weights import formula_state_dict
    from tests.util import golden_inputs
    cfg = GeneratorConfig(basechannels=8, depths=(2, 0, 2), num_heads=4)
    m = build_model(cfg, formula_state_dict(cfg), 'cuda:0')
    a = golden_inputs(3, 1, 5, 184, 240, 900)
    b = golden_inputs(3, 1, 5, 184, 240, 950)
    ya = torch.stack(m([{'events': torch.from_numpy(x).cuda()} for x in a]))
    yb = torch.stack(m([{'events': torch.from_numpy(x).cuda()} for x in b]))
    yab = torch.stack(m([{'events': torch.from_numpy(np.concatenate([x, y])).cuda()} for x, y in zip(a, b)]))
    # not bit-exact: the GEMM decomposition (split-K factor) is chosen from the launch size, so the
    # fp32 summation order differs between B=1 and B=2
    assert maxabs(yab[:, 0:1], ya) <= 2e-5
    assert maxabs(yab[:, 1:2], yb) <= 2e-5


def test_bad_shapes_raise():
    from bde2vid_amd.model import build_model
    from bde2vid_amd.config import GeneratorConfig
    from bde2vid_amd.weights import formula_state_dict
    cfg = GeneratorConfig(basechannels=8, depths=(2, 0, 2), num_heads=4)
    m = build_model(cfg, formula_state_dict(cfg), 'cuda:0')
    with pytest.raises(RuntimeError):     # not a multiple of 2^3
        m([{'events': torch.zeros(1, 5, 60, 64, device='cuda')}])
    with pytest.raises(RuntimeError):     # 32x40 -> 4x5 map at level 2 < 7x7 window (reference raises too)
        m([{'events': torch.zeros(1, 5, 32, 40, device='cuda')}])


@pytest.mark.parametrize('hw,T,B', [((260, 346), 3, 2), ((480, 640), 2, 1)])
def test_baseline_resolutions_vs_oracle(hw, T, B):
    """BASELINE.json configs[2..3] resolutions (DAVIS346 padded to 264x352 through Croper, VGA) with a
    small-channel model so the CPU oracle finishes in seconds; exercises row-tiled convs, multi-tile
    rows in the recurrent kernel and non-multiple-of-7 attention maps."""
    from bde2vid_amd.model import build_model
    from bde2vid_amd.config import GeneratorConfig
    from bde2vid_amd.weights import formula_state_dict
    from bde2vid_amd.harness import reconstruct_sequence, Croper
    from oracle import bde2vid_oracle as O
    from tests.util import voxel_like
    cfg = GeneratorConfig(basechannels=8, depths=(1, 0, 2), num_heads=4)
    sd = formula_state_dict(cfg)
    m = build_model(cfg, sd, 'cuda:0')
    vox = [torch.from_numpy(voxel_like((B, 5, hw[0], hw[1]), 1200 + t)) for t in range(T)]
    got = torch.stack(reconstruct_sequence(m, [v.cuda() for v in vox])).cpu()
    crop = Croper(3)
    crop.update_params(hw[1], hw[0])
    with torch.no_grad():
        ref = torch.stack([crop.crop(y) for y in O.forward(sd, cfg, [{'events': crop.pad(v)} for v in vox])])
    assert got.shape == ref.shape == (T, B, 1, hw[0], hw[1])
    assert maxabs(got, ref) <= TOL


def test_hd_frame_runs_and_is_finite():
    """Largest BASELINE size (720x1280): shape/LDS limits of every kernel, output in (0,1)."""
    from bde2vid_amd.model import build_model
    from bde2vid_amd.config import GeneratorConfig
    from bde2vid_amd.weights import formula_state_dict
    from tests.util import voxel_like
    cfg = GeneratorConfig(basechannels=8, depths=(1, 0, 1), num_heads=4)
    m = build_model(cfg, formula_state_dict(cfg), 'cuda:0')
    y = torch.stack(m([{'events': torch.from_numpy(voxel_like((1, 5, 720, 1280), 1300 + t)).cuda()} for t in range(2)]))
    assert tuple(y.shape) == (2, 1, 1, 720, 1280)
    assert torch.isfinite(y).all() and float(y.min()) >= 0.0 and float(y.max()) <= 1.0
    assert float(y.std()) > 0.01


def test_chunking_changes_only_chunk_edges_like_reference():
    """subseq_L chunking (eval_models_seq.py:216-219): every chunk starts from zero state, so running
    two chunks equals two independent forwards (and differs from one long forward)."""
    from bde2vid_amd.model import build_model
    from bde2vid_amd.config import GeneratorConfig
    from bde2vid_amd.weights import formula_state_dict
    from bde2vid_amd.harness import reconstruct_sequence
    from tests.util import voxel_like
    cfg = GeneratorConfig(basechannels=8, depths=(2, 0, 2), num_heads=4)
    m = build_model(cfg, formula_state_dict(cfg), 'cuda:0')
    vox = [torch.from_numpy(voxel_like((1, 5, 56, 64), 1400 + t)).cuda() for t in range(6)]
    whole = torch.stack(reconstruct_sequence(m, vox, subseq_L=None))
    chunks = torch.stack(reconstruct_sequence(m, vox, subseq_L=3))
    a = torch.stack(m([{'events': v} for v in vox[:3]]))
    b = torch.stack(m([{'events': v} for v in vox[3:]]))
    assert torch.equal(chunks, torch.cat([a, b]))
    assert maxabs(whole, chunks) > 1e-3


def test_pipelined_graph_mode_is_bit_identical():
    """Serving mode (3 sequences in flight, hipGraph replay) must return exactly what the plain
    eager, one-at-a-time mode returns for every sequence."""
    from bde2vid_amd.model import build_model
    from bde2vid_amd.config import GeneratorConfig
    from bde2vid_amd.weights import formula_state_dict
    from tests.util import golden_inputs
    cfg = GeneratorConfig(basechannels=8, depths=(2, 0, 2), num_heads=4)
    m = build_model(cfg, formula_state_dict(cfg), 'cuda:0')
    seqs = [[{'events': torch.from_numpy(x).cuda()} for x in golden_inputs(4, 1, 5, 64, 72, 1500 + 10 * i)]
            for i in range(7)]
    m.set_tuning('graph', 0)
    ref = [torch.stack(m(s)).clone() for s in seqs]
    m.set_tuning('graph', 1)
    m.set_tuning('pipeline', 3)
    outs = [m(s) for s in seqs]          # slots warm up, capture and replay along the way
    m.wait()
    torch.cuda.synchronize()
    for r, o in zip(ref, outs):
        assert torch.equal(r, torch.stack(o))
    m.set_tuning('pipeline', 1)


def test_checkpoint_file_round_trip(tmp_path):
    """A file in the reference's checkpoint format ({'state_dict', 'meta': {'cfg': <config source>}},
    eval_models_seq.py:52-60) loads without mmengine and reproduces the golden frames."""
    from bde2vid_amd.checkpoint import load_model
    z, meta = load_golden('e2e_tiny')
    cfg, sd, xs = case_from_meta(meta)
    src = ("model = dict(type='BDE2VID', cpu_cache_length=100, generator=dict(type='BDE2VIDCrossscalePropogationV5', "
           f"num_bins={cfg.num_bins}, basechannels={cfg.basechannels}, num_encoders={cfg.num_encoders}, ks={cfg.ks}, "
           f"num_res_blocks=2, norm=None, activation=dict(type='Sigmoid'), buffer_index={list(cfg.buffer_index)}, "
           f"q_idx={cfg.q_idx}, depths={list(cfg.depths)}, num_heads={cfg.num_heads}, losses=[]))")
    path = tmp_path / 'BDE2VID_epoch_1.pth'
    torch.save({'state_dict': sd, 'meta': {'cfg': src}}, str(path))
    m = load_model(str(path), 'cuda:0')
    with torch.no_grad():
        y = torch.stack(m([{'events': torch.from_numpy(x).cuda()} for x in xs]))
    assert maxabs(y, z['out']) <= TOL


def test_example_recording_to_frames(monkeypatch):
    """examples/reconstruct_recording.py end to end: native event columns -> windows -> chunks -> cropped frames."""
    import importlib.util, os, sys
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'reconstruct_recording.py')
    spec = importlib.util.spec_from_file_location('reconstruct_recording', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, 'argv', ['reconstruct_recording.py', '--frames', '6', '--height', '60', '--width', '72', '--subseq', '4'])
    out = mod.main()
    assert tuple(out.shape) == (6, 1, 60, 72)
    assert torch.isfinite(out).all() and float(out.min()) > 0.0 and float(out.max()) < 1.0


def test_long_sequence_more_frames_than_one_pointer_block():
    """T = 70 > 64: the frame gather / scatter launches take the frame pointers 64 at a time; outputs against the oracle."""
    from oracle import bde2vid_oracle as O
    z, meta = load_golden('e2e_tiny')
    from bde2vid_amd.model import build_model
    cfg, sd, xs = case_from_meta(meta)
    rng = np.random.default_rng(5)
    B, C, H, W = xs[0].shape
    frames = [(rng.standard_normal((B, C, H, W)).astype(np.float32) * 0.5 * (rng.random((B, C, H, W)) > 0.7)).astype(np.float32)
              for _ in range(70)]
    m = build_model(cfg, sd, 'cuda:0')
    with torch.no_grad():
        ys = torch.stack(m([{'events': torch.from_numpy(x).cuda()} for x in frames]))
        ref = torch.stack(O.forward(sd, cfg, [{'events': torch.from_numpy(x)} for x in frames]))
    assert tuple(ys.shape) == tuple(ref.shape)
    assert maxabs(ys, ref) <= TOL


@pytest.mark.parametrize('name', sorted(CFGA_SAMPLED))
def test_config_a_at_baseline_resolutions(name):
    """Canonical channel widths / heads / depths (the kernels bench.py times: winblock, wide_core, lstm16<1,128,2>,
    every conv_vec tile shape) at every BASELINE.json resolution and at bench.py's T=16, against the REFERENCE's
    outputs (sampled pixels + per-frame mean/std, oracle/gen_golden.py::gen_cfgA_sampled)."""
    z, meta = load_golden(name)
    m, cfg, sd, xs, y = run_case(meta)
    assert_sampled(y, z, meta, TOL, 1e-5)
    del m
    torch.cuda.empty_cache()


def test_bench_workload_matches_reference_in_serving_mode():
    """bench.py's exact workload and mode: voxel grids from the HIP scatter of the synthetic events, three sequences
    in flight, launch sequence replayed from hipGraphs -- every one of 7 calls must reproduce the reference's frames."""
    from bde2vid_amd import canonical
    from bde2vid_amd.model import build_model
    from bde2vid_amd.weights import formula_state_dict
    from bde2vid_amd.workload import bench_voxels, verify_against_fixture, find_fixture
    z, meta = load_golden('e2e_bench_T16')
    fixture_path, fmeta = find_fixture(meta['T'], meta['B'], meta['H'], meta['W'], meta['sensor'])
    assert fmeta == meta
    cfg = canonical()
    m = build_model(cfg, formula_state_dict(cfg, meta['weight_seed']), 'cuda:0')
    vox, n_events, _ = bench_voxels(meta['T'], tuple(meta['sensor']), 'cuda:0', seed0=meta['seed'])
    assert n_events == meta['T'] * meta['events_per_frame']
    inputs = [{'events': vox[t]} for t in range(meta['T'])]
    m.set_tuning('pipeline', 3)
    outs = [m(inputs) for _ in range(7)]
    m.wait()
    torch.cuda.synchronize()
    assert m.get_info('graphs_live') == 3
    for o in outs:
        y = torch.stack(o)
        assert_sampled(y, z, meta, TOL, 1e-5)
        ok, err = verify_against_fixture(y, fixture_path)
        assert ok and err <= TOL
    m.set_tuning('pipeline', 1)


@pytest.mark.parametrize('name', ['e2e_bench_480x640_T32_B4', 'e2e_bench_720x1280_T64'])
def test_baseline_configs_3_and_5_at_full_size(name):
    """BASELINE.json configs 3 and 5 at their FULL sizes (VGA T=32 B=4 with four different streams in the batch; HD T=64):
    the gate x-part workspace alone is 5.0e9 / 7.5e9 floats there, past 2^31 elements, so every index product of the path
    is exercised where an `int` would wrap.  Inputs = bench.py's workload (HIP binning of the synthetic events); expected =
    what the REFERENCE computed for the same events in the build container (oracle/gen_golden.py::gen_bench_fullsize):
    pixels at stride 16 plus per-frame mean / std.  Eager call, then the graph replay of the same shape."""
    from bde2vid_amd import canonical
    from bde2vid_amd.model import build_model
    from bde2vid_amd.weights import formula_state_dict
    from bde2vid_amd.workload import bench_voxels, verify_against_fixture, find_fixture
    z, meta = load_golden(name)
    cfg = canonical()
    m = build_model(cfg, formula_state_dict(cfg, meta['weight_seed']), 'cuda:0')
    T, B = meta['T'], meta['B']
    vox, n_events, _ = bench_voxels(T, tuple(meta['sensor']), 'cuda:0', seed0=meta['seed'], batch=B)
    assert n_events == T * B * meta['events_per_frame'] and tuple(vox.shape) == (T, B, 5, meta['H'], meta['W'])
    inputs = [{'events': vox[t]} for t in range(T)]
    path, fmeta = find_fixture(T, B, meta['H'], meta['W'], meta['sensor'])
    assert fmeta == meta
    with torch.no_grad():
        for rep in range(3):                              # eager, capture, replay
            y = torch.stack(m(inputs))
            torch.cuda.synchronize()
            assert_sampled(y, z, meta, TOL, 1e-5)
            ok, err = verify_against_fixture(y, path)
            assert ok and err <= TOL, (rep, err)
            del y
    assert m.get_info('graphs_live') == 1
    del m
    torch.cuda.empty_cache()


@pytest.mark.parametrize('name', sorted(LONGT_CASES))
def test_longer_than_cpu_cache_length(name):
    """T > cpu_cache_length (V5.py:102): the reference parks feature maps on the host; here everything stays in HBM
    (the constructor argument is accepted and ignored).  Reference outputs, T = 7 with cache 3 and T = 104 with 100."""
    from bde2vid_amd.model import BDE2VID
    z, meta = load_golden(name)
    cfg, sd, xs = case_from_meta(meta)
    m = BDE2VID(generator=cfg, cpu_cache_length=meta['cpu_cache_length']).to('cuda:0')
    m.load_state_dict(sd)
    with torch.no_grad():
        y = torch.stack(m([{'events': torch.from_numpy(x).cuda()} for x in xs]))
    assert_sampled(y, z, meta, TOL, 1e-5)


def test_pipelined_mode_with_temporaries_and_dropped_outputs():
    """Serving mode with inputs that need a .contiguous() copy and outputs the caller drops at once: the library's
    internal streams must still see valid memory (the tensors are recorded on those streams)."""
    from bde2vid_amd.model import build_model
    from bde2vid_amd.config import GeneratorConfig
    from bde2vid_amd.weights import formula_state_dict
    from tests.util import golden_inputs
    cfg = GeneratorConfig(basechannels=8, depths=(2, 0, 2), num_heads=4)
    m = build_model(cfg, formula_state_dict(cfg), 'cuda:0')
    seqs = []
    for i in range(6):
        xs = golden_inputs(4, 1, 5, 64, 72, 1700 + 10 * i)
        # channel-last storage: [B,5,H,W] views that are NOT contiguous
        seqs.append([{'events': torch.from_numpy(x).cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)} for x in xs])
        assert not seqs[-1][0]['events'].is_contiguous()
    ref = [torch.stack(m(s)).clone() for s in seqs]
    m.set_tuning('pipeline', 3)
    keep = []
    for rep in range(3):
        for i, s in enumerate(seqs):
            o = m(s)
            if rep == 2:
                keep.append(o)
            else:
                del o                                        # dropped while still in flight
            junk = torch.full((4, 1, 1, 64, 72), float('nan'), device='cuda')   # grabs freshly freed blocks if any
            del junk
    m.wait()
    torch.cuda.synchronize()
    for r, o in zip(ref, keep):
        assert torch.equal(r, torch.stack(o))
    m.set_tuning('pipeline', 1)


def test_broadcast_receiver_path_on_one_gpu():
    """What ranks 1..N-1 run (dist.build_replicated_model): allocate the packed layout without weights, receive the
    image, compute.  Here the 'broadcast' is a device copy from a model packed the ordinary way."""
    from bde2vid_amd.model import BDE2VID, build_model
    z, meta = load_golden('e2e_tiny')
    cfg, sd, xs = case_from_meta(meta)
    a = build_model(cfg, sd, 'cuda:0')
    b = BDE2VID(generator=cfg).to('cuda:0').alloc_packed()
    va, vb = a.packed_view(), b.packed_view()
    assert va.shape == vb.shape and va.data_ptr() != vb.data_ptr()
    vb.copy_(va)
    inp = [{'events': torch.from_numpy(x).cuda()} for x in xs]
    ya, yb = torch.stack(a(inp)), torch.stack(b(inp))
    assert torch.equal(ya, yb)
    assert maxabs(yb, z['out']) <= TOL


def test_single_rank_rccl_broadcast_through_build_replicated_model(monkeypatch):
    """dist.build_replicated_model over the nccl (= RCCL) backend with one rank: the collective call itself runs."""
    import socket
    import torch.distributed as dist
    from bde2vid_amd.dist import init_from_env, build_replicated_model
    z, meta = load_golden('e2e_tiny')
    cfg, sd, xs = case_from_meta(meta)
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = str(sk.getsockname()[1])
    for k, v in dict(BDE_FORCE_DIST='1', WORLD_SIZE='1', RANK='0', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1',
                     MASTER_PORT=port).items():
        monkeypatch.setenv(k, v)
    rank, world, local = init_from_env('nccl')
    try:
        m = build_replicated_model(cfg, lambda: sd, torch.device('cuda', local))
        with torch.no_grad():
            y = torch.stack(m([{'events': torch.from_numpy(x).cuda()} for x in xs]))
        assert maxabs(y, z['out']) <= TOL
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_bench_two_ranks_on_one_gpu_over_gloo():
    """bench.py's multi-rank path end to end (rank 0 packs, rank 1 allocates the packed layout and receives the image by
    the collective, both reconstruct and check their frames against the reference fixture), two processes on this one
    GPU with the gloo backend: what the 8-GPU run does over RCCL."""
    import json, os, subprocess, sys, socket
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = str(sk.getsockname()[1])
    env = dict(os.environ, BDE_DIST_BACKEND='gloo', MASTER_ADDR='127.0.0.1', MASTER_PORT=port)
    env.pop('WORLD_SIZE', None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
           '--master-port', port, os.path.join(repo, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1', '--pipeline', '2',
           '--no-cpu-baseline']
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('{')][-1]
    d = json.loads(line)
    assert d['n_gpus'] == 2 and d['verified'] is True and d['verification']['max_abs_err'] <= 2e-4


def test_nan_voxel_grid_gives_the_reference_nan_frames():
    """A zero-duration event window makes the reference's voxel grid NaN (event_utils.py:489-495), and -- torch's ReLU /
    ReLU6 hand a NaN on, the recurrence and the window attention spread it -- every frame of the sequence NaN (checked on
    the oracle in the build container: 100 % of the pixels of all five frames).  The same must happen here: a max()-based
    activation would silently turn the NaN into a zero and return plausible-looking frames."""
    from oracle import bde2vid_oracle as O
    from bde2vid_amd.model import build_model
    z, meta = load_golden('e2e_tiny')
    cfg, sd, xs = case_from_meta(meta)
    xs = [x.copy() for x in xs]
    xs[2][0, :, 20:23, 30:34] = np.nan                                      # a patch of frame 2
    m = build_model(cfg, sd, 'cuda:0')
    with torch.no_grad():
        y = torch.stack(m([{'events': torch.from_numpy(x).cuda()} for x in xs])).cpu()
        ref = torch.stack(O.forward(sd, cfg, [{'events': torch.from_numpy(x)} for x in xs]))
    assert torch.isnan(ref).all()
    assert torch.equal(torch.isnan(y), torch.isnan(ref))
    # and the model object is not poisoned: the next call on clean inputs reproduces the golden frames
    with torch.no_grad():
        xs2 = case_from_meta(meta)[2]
        y2 = torch.stack(m([{'events': torch.from_numpy(x).cuda()} for x in xs2]))
    assert maxabs(y2, z['out']) <= TOL


_SPLIT_WORKER = r'''
import json, os, sys, torch
sys.path.insert(0, %r)
import torch.distributed as dist
from bde2vid_amd.dist import init_from_env, DirectionSplit
from bde2vid_amd.model import build_model
from tests.util import load_golden, case_from_meta, maxabs
rank, world, local = init_from_env('gloo')
assert world == 2
report = {}
for name in %r:
    z, meta = load_golden(name)
    cfg, sd, xs = case_from_meta(meta)
    m = build_model(cfg, sd, 'cuda:0')
    inputs = [{'events': torch.from_numpy(x).cuda()} for x in xs]
    split = DirectionSplit(m, ranks=(0, 1))
    with torch.no_grad():
        ys = split(inputs)
        ys2 = split(inputs)                       # a second call on the same workspaces
        torch.cuda.synchronize()
        if rank == 0:
            joint = torch.stack(m(inputs))        # the ordinary single-GPU forward, same model object
            y, y2 = torch.stack(ys), torch.stack(ys2)
            report[name] = dict(equal=bool(torch.equal(y, joint)), repeat=bool(torch.equal(y, y2)),
                                err=maxabs(y, z['out']))
        else:
            assert ys is None and ys2 is None
    dist.barrier()
if rank == 0:
    open(os.path.join(%r, 'report.json'), 'w').write(json.dumps(report))
dist.destroy_process_group()
'''


def test_one_sequence_split_over_two_ranks_by_direction(tmp_path):
    """f-4, SURVEY.md §8(e) option 1: forward sweeps, merge, attention and decoder on rank 0, backward sweeps on rank 1, two
    tensors exchanged per level (dist.DirectionSplit over bde_split_*).  Two processes on this one GPU over gloo -- what two
    MI355X do over RCCL.  Rank 0's frames must equal the ordinary single-GPU forward BIT FOR BIT (every launch is the joint
    forward's launch for that direction) and match the reference's golden frames: ConvLSTM with both attention kernels'
    configurations, T = 1, batch 2, ConvGRU, and the bottleneck variant."""
    import json, os, socket, subprocess, sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = ['e2e_tiny', 'e2e_cfgA_small', 'e2e_T1', 'e2e_B2', 'e2e_buf5', 'var_convgru', 'var_bottleneck', 'var_norc']
    script = tmp_path / 'split_worker.py'
    script.write_text(_SPLIT_WORKER % (repo, names, str(tmp_path)))
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = str(sk.getsockname()[1])
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=port, HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('WORLD_SIZE', None)
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
                        '--master-port', port, str(script)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rep = json.loads((tmp_path / 'report.json').read_text())
    assert sorted(rep) == sorted(names)
    for name, v in rep.items():
        assert v['equal'], f'{name}: split frames differ from the single-GPU forward'
        assert v['repeat'], f'{name}: second split call differs'
        assert v['err'] <= TOL, (name, v['err'])


def test_switched_kernels_agree_with_the_default_build():
    """The split-operand recurrent step (lstm_sb.h), the split GEMM phases of the attention block (winblock_sb.h), the fp32
    chain of the level-2 attention (wideblock.h: wide_kv_sb, wide_fuse_mlp), the two-stream sweep option, the x-part of the gates inside the step, the operand
    format (two fp16 terms vs three bf16 terms) and the split convolutions altogether: each switched in turn must give the
    frames of the default build to fp32 rounding (canonical config, 184x240, T = 6) -- and all of them match the reference's
    golden frames through the other tests."""
    from tests.util import golden_inputs
    from bde2vid_amd import canonical
    from bde2vid_amd.model import build_model
    from bde2vid_amd.weights import formula_state_dict
    cfg = canonical()
    m = build_model(cfg, formula_state_dict(cfg), 'cuda:0')
    xs = golden_inputs(6, 1, 5, 184, 240, 2468)
    inp = [{'events': torch.from_numpy(x).cuda()} for x in xs]
    with torch.no_grad():
        base = torch.stack(m(inp)).clone()
        assert [m.get_info(f'sb_lstm{l}') for l in range(3)] == [1, 1, 1]
        terms = m.get_info('sb_terms')                                 # 2 unless BDE_SB_TERMS says otherwise
        for key, off, on in (('lstm_sbk', 0, 1), ('winblock_sb', 0, 1), ('lstm_two_streams', 1, 0),
                             ('lstm_fuse_x', 0, 1), ('sb_terms', 5 - terms, terms), ('conv_sb', 0, 1), ('wide_kv_sb', 0, 1), ('wide_fuse_mlp', 0, 1), ('head3', 0, 1)):
            m.set_tuning(key, off)
            try:
                y = torch.stack(m(inp))
                y2 = torch.stack(m(inp))                       # second call: the captured graph of the switched schedule
            finally:
                m.set_tuning(key, on)
            assert maxabs(y, base) <= 2e-5, key
            assert torch.equal(y, y2), key
        last = torch.stack(m(inp))
        assert torch.equal(last, base), maxabs(last, base)
        assert m.get_info('head3') == 1


def _scaled_head_model(scale):
    """Canonical config, formula weights, the head convolution scaled so that level-0 activations pass 65520."""
    from bde2vid_amd import canonical
    from bde2vid_amd.model import build_model
    from bde2vid_amd.weights import formula_state_dict
    cfg = canonical()
    sd = {k: v.clone() for k, v in formula_state_dict(cfg).items()}
    for k in ('generator.head.conv2d.weight', 'generator.head.conv2d.bias'):
        sd[k] = sd[k] * scale
    return cfg, sd, build_model(cfg, sd, 'cuda:0')


def test_range_guard_recomputes_with_three_terms():
    """The default operand format (two fp16 terms, csrc/split.h) carries finite activations below 65520 only; the reference
    computes in fp32 (submodules.py:105-114, 316-332).  With head weights scaled so that level-0 feature maps pass that limit the
    forward is detected on the device and recomputed with three bf16 terms: the caller gets the frames of the sb_terms = 3 build,
    not NaNs, the model keeps that format, and an ordinary model is left alone."""
    from tests.util import golden_inputs
    if int(__import__('os').environ.get('BDE_SB_TERMS', 2)) != 2:
        pytest.skip('the guard belongs to the two-term format')
    xs = golden_inputs(2, 1, 5, 184, 240, 4321)
    inp = [{'events': torch.from_numpy(x).cuda()} for x in xs]
    cfg, sd, m = _scaled_head_model(3.0e5)
    with torch.no_grad():
        assert m.get_info('sb_terms') == 2 and m.get_info('sb_auto') == 1
        y = torch.stack(m(inp)).clone()
        assert m.get_info('sb_overflows') == 1 and m.get_info('sb_latched') == 1 and m.get_info('sb_terms') == 3
        head = m.get_intermediate('head', (2, 1, cfg.basechannels, 184, 240))
        assert float(head.max()) > 65520.0                              # the premise: a level-0 activation beyond fp16
        y_again = torch.stack(m(inp))                                   # the latched format: no further recomputation
        assert m.get_info('sb_overflows') == 1
    _, _, m3 = _scaled_head_model(3.0e5)
    m3.set_tuning('sb_terms', 3)
    with torch.no_grad():
        ref = torch.stack(m3(inp))
    assert torch.isfinite(y).all() and torch.isfinite(ref).all()
    assert maxabs(y, ref) <= 2e-5 and maxabs(y_again, ref) <= 2e-5
    assert float(ref.std()) > 1e-3                                       # not a saturated constant image
    # an ordinary model never trips the guard
    _, _, m1 = _scaled_head_model(1.0)
    with torch.no_grad():
        m1(inp)
        m1(inp)
    assert m1.get_info('sb_overflows') == 0 and m1.get_info('sb_terms') == 2 and m1.get_info('sb_latched') == 0


def test_range_guard_error_path_and_serving_mode():
    """"sb_auto" = 0: the same forward fails with BDE_ERR_RANGE instead (bde_forward in the default mode, bde_wait_outputs in
    serving mode) and the model stays in the two-term format.  Serving mode with "sb_auto" = 1: three sequences in flight, one
    of them with event counts large enough to overflow -- after wait() every sequence holds the frames of the three-term build."""
    from bde2vid_amd import _lib
    from tests.util import golden_inputs
    if int(__import__('os').environ.get('BDE_SB_TERMS', 2)) != 2:
        pytest.skip('the guard belongs to the two-term format')
    xs = golden_inputs(2, 1, 5, 184, 240, 4321)
    inp = [{'events': torch.from_numpy(x).cuda()} for x in xs]
    cfg, sd, m = _scaled_head_model(3.0e5)
    m.set_tuning('sb_auto', 0)
    with torch.no_grad():
        with pytest.raises(_lib.RangeError):
            m(inp)
        assert m.get_info('sb_terms') == 2 and m.get_info('sb_overflows') == 1
        m.set_tuning('pipeline', 2)
        m(inp)
        with pytest.raises(_lib.RangeError):
            m.wait()
        m.set_tuning('pipeline', 1)
    # serving mode, automatic: an ordinary model, one sequence of huge voxel counts among ordinary ones
    _, _, m2 = _scaled_head_model(1.0)
    big = [{'events': d['events'] * 2.0e6} for d in inp]
    seqs = [inp, inp, big, inp, big, inp, inp]
    _, _, m3 = _scaled_head_model(1.0)
    m3.set_tuning('sb_terms', 3)
    with torch.no_grad():
        ref = [torch.stack(m3(s)).clone() for s in seqs]
        m2.set_tuning('pipeline', 3)
        outs = [m2(s) for s in seqs]
        m2.wait()
        torch.cuda.synchronize()
        m2.set_tuning('pipeline', 1)
    assert m2.get_info('sb_latched') == 1 and m2.get_info('sb_overflows') >= 1
    for i, (r, o) in enumerate(zip(ref, outs)):
        o = torch.stack(o)
        assert torch.isfinite(o).all(), i
        # (sequences that ran before the switch keep their two-term frames: both formats are fp32-equivalent)
        assert maxabs(o, r) <= 2e-5, i


def test_forked_decoder_is_bit_identical_to_the_serial_schedule():
    """"overlap" = 1 (off by default: measured slower, a forked hipGraph does not replay as one batch on ROCm 7.2): the decoder of
    the frames already refined runs in chunks of four on a forked branch of the captured graph beside the last level's attention
    chain (V5.py:183-202 is independent per frame); the last chunk and the cut
    into eager head / graph / eager tail around the range guard's read-back are part of the same schedule.  Every launch is the
    launch of the serial schedule restricted to its frames: frames equal bit for bit, call after call, one sequence in flight or
    three (a forked schedule runs eagerly: csrc/api_schedule.h, forward_on)."""
    from tests.util import golden_inputs
    from bde2vid_amd import canonical
    from bde2vid_amd.model import build_model
    from bde2vid_amd.weights import formula_state_dict
    cfg = canonical()
    m = build_model(cfg, formula_state_dict(cfg), 'cuda:0')
    for T in (10, 5):
        xs = golden_inputs(T, 1, 5, 184, 240, 97531 + T)
        inp = [{'events': torch.from_numpy(x).cuda()} for x in xs]
        with torch.no_grad():
            m.set_tuning('overlap', 0)
            ref = torch.stack(m(inp)).clone()
            ref2 = torch.stack(m(inp)).clone()            # second call of the shape: the captured graph
            m.set_tuning('overlap', 1)
            outs = [torch.stack(m(inp)).clone() for _ in range(3)]
            m.set_tuning('pipeline', 3)
            pip = [m(inp) for _ in range(7)]
            m.wait()
            torch.cuda.synchronize()
            m.set_tuning('pipeline', 1)
            m.set_tuning('overlap', 0)
        assert torch.equal(ref, ref2)
        for o in outs:
            assert torch.equal(o, ref), T
        for o in pip:
            assert torch.equal(torch.stack(o), ref), T

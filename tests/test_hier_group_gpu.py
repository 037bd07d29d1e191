"""The hierarchical group term on the GPU: k_hier_pairs and the HierCe policy of the tile-queue core (csrc/online_plbl.hip) against the
library's host loop through csrc/hier_group.h (``ops.hier_group_loss_reference``) bit for bit -- the sums, the pair table, the fixed-point
gradient and its rounding --, at quarter resolution and in the full-resolution form, the modules against the executed reference
(tests/golden/g19_hier_group.npz), run-to-run identical bytes, the second id map through the file-backed loader, and the trainer end
to end."""
import logging
import os
import pickle
import random
import tempfile
import types

import numpy as np
import pytest
import torch

from mulactseg_amd import synth

import helpers
from test_hier_group_cpu import bits_of, cleared_rows, golden_case, small_map, with_last_column
from test_losses_gpu import _inputs

pytestmark = pytest.mark.gpu
# (N, C, h, w, H, W, S, Ss): the golden shape at quarter resolution, a non-integer scale, a ragged two-tile row
LOW = [(2, 20, 10, 11, 40, 44, 48, 12), (2, 20, 10, 11, 40, 44, 48, 192), (2, 21, 9, 10, 33, 37, 150, 40), (1, 20, 3, 75, 9, 300, 24, 60)]
_CASES = {}


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    return ops


def _case(shape):
    """Host tensors of a shape, made once: (zq, spx, small, msk, bits)."""
    if shape not in _CASES:
        N, C, h, w, H, W, S, Ss = shape
        _, tgt, spx, msk = _inputs(900 + W + C, N, C, H, W, S)
        zq = synth.logits(77 + h, N, C, h, w)
        _CASES[shape] = (torch.from_numpy(zq), torch.from_numpy(spx), torch.from_numpy(small_map(900 + W + C, spx, S, Ss)),
                         torch.from_numpy(msk), bits_of(tgt))
    return _CASES[shape]


def _equal_to_the_reference(ops, zq, size, spx, small, msk, bits, Ss, only_single, nocropsp, dtypes=(torch.int64,), empty=False):
    grad = torch.tensor([16.0], dtype=torch.float32)
    ref = ops.hier_group_loss_reference(zq, size, spx, small, Ss, msk, bits, only_single=only_single, nocropsp=nocropsp, grad=grad)
    if empty:           # every row cleared: nothing is counted, the loss is 0 and the gradient all zero
        assert int(ref['acc'][1]) == 0 and float(ref['loss']) == 0.0 and not bool(ref['dzq_fix'].any())
    else:
        assert int(ref['acc'][1]) > 0 and bool(ref['dzq_fix'].any())
    zg, mg, bg, gg = zq.cuda(), msk.cuda(), bits.cuda(), grad.cuda()
    for dt in dtypes:
        sg, fg = spx.to(dt).cuda(), small.to(dt).cuda()
        out = ops.hier_group_loss_fwd(zg, size, sg, fg, Ss, mg, bg, only_single=only_single, nocropsp=nocropsp)
        what = (tuple(zq.shape), size, Ss, only_single, nocropsp, dt)
        assert torch.equal(out['gmax'].cpu(), ref['gmax']), what
        assert torch.equal(out['mult'].cpu(), ref['mult']) and torch.equal(out['any'].cpu(), ref['any']), what
        assert torch.equal(out['acc'].cpu(), ref['acc']), what
        assert torch.equal(out['loss'].cpu().view(torch.int32), ref['loss'].view(torch.int32)), what
        if nocropsp:
            assert torch.equal(out['bits_eff'].cpu(), ref['bits_eff']) and torch.equal(bg.cpu(), bits), what
        dz, fix = ops.hier_group_loss_bwd(zg, size, fg, Ss, mg, out['mult'], out['any'], out['acc'], gg, want_fix=True)
        assert torch.equal(fix.cpu(), ref['dzq_fix']), what
        assert torch.equal(dz.cpu().view(torch.int32), ref['dz'].view(torch.int32)), what
    return ref


@pytest.mark.parametrize("shape", LOW)
@pytest.mark.parametrize("only_single", [False, True])
@pytest.mark.parametrize("nocropsp", [False, True])
def test_kernels_equal_the_host_reference_bit_for_bit(shape, only_single, nocropsp):
    ops = _gpu()
    N, C, h, w, H, W, S, Ss = shape
    zq, spx, small, msk, bits = _case(shape)
    dtypes = (torch.int64, torch.int32, torch.int16) if (only_single, nocropsp) == (False, False) else (torch.int64,)
    # in the nine rows of the ragged shape every superpixel touches the border: --nocropsp clears every row there
    _equal_to_the_reference(ops, zq, (H, W), spx, small, msk, bits, Ss, only_single, nocropsp, dtypes, empty=nocropsp and H == 9)


def test_a_pair_of_multiplicity_two_is_in_the_quarter_resolution_cases():
    ops = _gpu()
    N, C, h, w, H, W, S, Ss = LOW[0]
    zq, spx, small, msk, bits = _case(LOW[0])
    out = ops.hier_group_loss_fwd(zq.cuda(), (H, W), spx.cuda(), small.cuda(), Ss, msk.cuda(), bits.cuda())
    assert int(out['mult'].max()) >= 2


@pytest.mark.parametrize("Ss", [192, 12])
@pytest.mark.parametrize("key", ['hier_all', 'hier_single', 'aug_all', 'aug_single'])
def test_the_full_resolution_form_matches_the_reference_and_the_golden(Ss, key):
    """h = H, w = W: the taps are exactly (1, 0).  Bit for bit against the host loop; the modules against the executed reference at the
    tolerance of tests/test_hier_group_cpu.py (1e-4 * max(1, |ref|) for the loss, 1e-4 * max|ref| for the gradient, the count exactly)."""
    ops = _gpu()
    from mulactseg_amd.utils import loss as L
    g, z, tgt, spx, small, msk = golden_case(Ss)
    aug, single = key.startswith('aug'), key.endswith('single')
    k = "%s_%d" % (key, Ss)
    zc, sc, fc, mc = torch.from_numpy(z), torch.from_numpy(spx), torch.from_numpy(small), torch.from_numpy(msk)
    _equal_to_the_reference(ops, zc, None, sc, fc, mc, bits_of(tgt[..., :-1]), Ss, single, aug)
    cls = L.AugHierGroupMultiLabelCE if aug else L.HierGroupMultiLabelCE
    args = types.SimpleNamespace(small_nseg=Ss)
    zg = zc.cuda().requires_grad_(True)
    tg = torch.from_numpy(tgt).cuda()
    before = tg.clone()
    crit = cls(args, z.shape[1], tgt.shape[1], single, -1, temperature=0.1)
    loss = crit(zg, tg, mc.cuda(), sc.cuda(), fc.cuda())
    (float(g['weight']) * loss).backward()
    ref, gref = float(g[k + '_loss']), g[k + '_grad']
    err, scale = float(np.max(np.abs(zg.grad.cpu().numpy() - gref))), float(np.max(np.abs(gref)))
    print("g19 %s: loss %.7g golden %.7g, n %d golden %d, gradient error %.3e of %.3e"
          % (k, float(loss), ref, int(crit.last_acc[1]), int(g[k + '_n']), err, scale))
    assert int(crit.last_acc[1]) == int(g[k + '_n'])
    assert abs(float(loss) - ref) <= 1e-4 * max(1.0, abs(ref))
    assert scale > 0 and err <= 1e-4 * scale
    assert torch.equal(tg, before)                          # the caller's tensor is untouched
    s, n1 = cls(args, z.shape[1], tgt.shape[1], single, -1, reduction='none')(zc.cuda(), tg, mc.cuda(), sc.cuda(), fc.cuda())
    assert int(n1) == int(g[k + '_n']) + 1 and abs(float(s) / int(n1) - ref) <= 1e-4 * max(1.0, abs(ref))
    if aug and not single and Ss == 12:                     # both terms see the cleared rows
        pos = crit.merged_positive(zc.cuda(), None, sc.cuda(), mc.cuda(), float(g['pos_temp']))
        assert abs(float(pos) - float(g['aug_pos_loss'])) <= 1e-4 * max(1.0, abs(float(g['aug_pos_loss'])))
        assert torch.equal(crit.last_bits.cpu(), bits_of(cleared_rows(tgt, spx, tgt.shape[1])[..., :-1]))


def test_lowres_equals_the_materialised_upsample():
    ops = _gpu()
    N, C, h, w, H, W, S, Ss = LOW[2]
    zq, spx, small, msk, bits = _case(LOW[2])
    zg, sg, fg, mg, bg = zq.cuda(), spx.cuda(), small.cuda(), msk.cuda(), bits.cuda()
    low = ops.hier_group_loss_fwd(zg, (H, W), sg, fg, Ss, mg, bg)
    full = ops.hier_group_loss_fwd(ops.upsample_bilinear(zg, (H, W)), None, sg, fg, Ss, mg, bg)
    assert int(low['acc'][1]) > 0
    for k in ('acc', 'mult', 'any', 'gmax'):
        assert torch.equal(low[k], full[k]), k


def test_two_launches_leave_identical_bytes():
    ops = _gpu()
    N, C, h, w, H, W, S, Ss = LOW[0]
    zq, spx, small, msk, bits = _case(LOW[0])
    zg, sg, fg, mg, bg = zq.cuda(), spx.cuda(), small.cuda(), msk.cuda(), bits.cuda()
    gg = torch.tensor([16.0], dtype=torch.float32).cuda()
    runs = []
    for _ in range(2):
        out = ops.hier_group_loss_fwd(zg, (H, W), sg, fg, Ss, mg, bg, nocropsp=True)
        dz, fix = ops.hier_group_loss_bwd(zg, (H, W), fg, Ss, mg, out['mult'], out['any'], out['acc'], gg, want_fix=True)
        runs.append([out[k].clone() for k in ('acc', 'mult', 'any', 'gmax', 'bits_eff', 'loss')] + [dz, fix])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_forward_lowres_builds_no_full_resolution_tensor():
    _gpu()
    from mulactseg_amd.utils import loss as L
    N, C, h, w, H, W, S, Ss = 2, 19, 48, 48, 192, 192, 64, 256
    _, tgt, spx, msk = _inputs(5, N, C, H, W, S)
    crit = L.HierGroupMultiLabelCE(types.SimpleNamespace(small_nseg=Ss), C, S, False, -1)
    zq = torch.from_numpy(synth.logits(6, N, C, h, w)).cuda().requires_grad_(True)
    tg, sp, mk = torch.from_numpy(with_last_column(tgt)).cuda(), torch.from_numpy(spx).cuda(), torch.from_numpy(msk).cuda()
    sm = torch.from_numpy(small_map(5, spx, S, Ss)).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    group = crit.forward_lowres(zq, (H, W), tg, mk, sp, sm)
    pos = crit.merged_positive(zq, (H, W), sp, mk, 0.1)
    (16.0 * pos + group).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("peak allocation of a forward_lowres step: %d bytes; one [N,C,H,W] f32 tensor: %d bytes" % (peak, N * C * H * W * 4))
    assert peak < N * C * H * W * 4 and float(group) > 0 and float(zq.grad.abs().max()) > 0


def test_the_loader_carries_the_second_map_through_the_augmentation(tmp_path):
    """The stored fine map is 2 * spx + (x & 1) with small_nseg = 2 * nseg: whatever scale, pad, crop and flip a sample draws, both
    maps must have gone through the same geometry, pads included (small_nseg // 2 == nseg)."""
    _gpu()
    from mulactseg_amd import dataloader
    dataloader.register_dataset_factory(None)
    H, W, NSEG, CROP = 96, 160, 64, 128
    tree = helpers.write_cityscapes_tree(str(tmp_path / 'data'), n=3, H=H, W=W, nseg=NSEG)
    fine_dir = os.path.join(tree['root'], 'superpixel_seed/cityscapes/seeds_%d/train/label' % (2 * NSEG))
    os.makedirs(fine_dir)
    for stem, spx in zip(tree['stems'], tree['spx']):
        fine = (2 * spx + (np.arange(W)[None, :] & 1)).astype(np.int32)
        with open(os.path.join(fine_dir, stem + '.pkl'), 'wb') as f:
            pickle.dump({'labels': fine, 'valid_idxes': np.unique(fine)}, f)
    args = helpers.cityscapes_tree_args(tree, tmp_path / 'run', ['--method', 'active_joint_hier_multi', '--load_smaller_spx', '--small_nseg',
                                                                 str(2 * NSEG)])
    os.makedirs(args.model_save_dir, exist_ok=True)
    aset = dataloader.get_active_dataset(args, train_transform=args.train_transform)
    pool, label = aset.trg_pool_dataset, aset.trg_label_dataset
    assert label.transform.n_maps == 2 and label.transform.pad_values == [NSEG, 2 * NSEG]
    label.transform.size = (CROP, CROP)
    assert 'spx_small' not in pool[0]                       # pool samples are unchanged
    aset.selection_iter = 1
    sel = [3, 7, 11, 40]
    aset.expand_training_set([(1.0 - 0.01 * i, ','.join(pool.im_idx[1]), s) for i, s in enumerate(sel)], 10 ** 6, 'x')
    assert ('ids', label.small_spx_fname(label.im_idx[0][2])) in label.sample_files(0)      # prefetched with the sample
    label.transform.rng = random.Random(11)
    pads = parity = 0
    for _ in range(4):
        s = label[0]
        spx, small = s['spx'], s['spx_small']
        assert tuple(small.shape) == tuple(spx.shape) == (CROP, CROP) and small.is_cuda
        assert torch.equal(small // 2, spx)
        pads += int((spx == NSEG).sum())
        parity += int((small[spx < NSEG] & 1).sum())
        assert torch.equal(s['spmask'].cpu(), torch.from_numpy(np.isin(spx.cpu().numpy(), sel)))
    assert pads > 0 and parity > 0                          # padded draws and both halves of the fine ids were seen


class _Train(torch.utils.data.Dataset):
    """Two 128 x 128 samples with a fine map of 256 ids."""
    H = W = 128
    S, Ss, cols = 64, 256, 20

    def __init__(self):
        self.selection_iter = 1

    def __len__(self):
        return 2

    def __getitem__(self, i):
        rs = np.random.RandomState(100 + i)
        spx, msk = synth.train_crop(200 + i, self.H, self.W, self.S, frac_selected=0.3)
        return {'images': torch.from_numpy(rs.standard_normal((3, self.H, self.W)).astype(np.float32)),
                'labels': torch.from_numpy(synth.multi_hot_targets(300 + i, self.S, self.cols)),
                'spx': torch.from_numpy(spx), 'spmask': torch.from_numpy(msk),
                'spx_small': torch.from_numpy(small_map(400 + i, spx[None], self.S, self.Ss)[0])}


class _Val(torch.utils.data.Dataset):
    def __len__(self):
        return 1

    def __getitem__(self, i):
        return {'images': torch.zeros((3, 128, 128)), 'labels': torch.zeros((128, 128), dtype=torch.int64)}


@pytest.mark.parametrize("extra", [[], ['--nocropsp', '--group_only_single']])
def test_the_trainer_runs_a_quarter_resolution_step(extra):
    _gpu()
    import importlib
    from mulactseg_amd import dataloader
    from mulactseg_amd.utils import common, loss as L
    method = 'active_joint_hier_multi'
    a = common.get_parser().parse_args([
        '-m', 'deeplabv3pluswn_resnet50deepstem', '--separable_conv', '--method', method, '--ce_temp', '0.1', '--multi_ce_temp', '0.1',
        '--group_ce_temp', '0.1', '--coeff', '16.0', '--or_labeling', '--fair_counting', '--nseg', str(_Train.S), '--load_smaller_spx',
        '--small_nseg', str(_Train.Ss), '--train_batch_size', '2', '--val_batch_size', '1', '--num_workers', '0', '--val_num_workers', '0',
        '--train_lr', '2e-5', '--finetune_itrs', '2', '--val_period', '1000', '--log_period', '1', '-p', tempfile.mkdtemp()] + extra)
    a.pretrained_backbone = False
    a.lowres_loss = True
    dataloader.register_dataset_factory(lambda args, name, data_root, datalist, imageset: _Val())
    torch.manual_seed(0)
    tr = importlib.import_module("mulactseg_amd.trainer." + method).ActiveTrainer(a, logging.getLogger("test"), 1)
    tr._wandb_log = lambda payload, step: None
    assert type(tr.hier_group_multi_loss) is (L.AugHierGroupMultiLabelCE if extra else L.HierGroupMultiLabelCE)
    assert tr.hier_group_multi_loss.only_single is bool(extra) and tr.num_classes == 19
    seen = dict(lowres=[], meters=[])
    fwd, meter_fn = tr.forward_train, tr.update_average_meter

    def forward_train(images, **kw):
        seen['lowres'].append(kw.get('lowres', False))
        out = fwd(images, **kw)
        assert out.shape[1] == 19 and tuple(out.shape[-2:]) == (32, 32)
        return out

    def update_average_meter(values):
        seen['meters'].append({k: v.detach().clone() for k, v in values.items()})
        return meter_fn(values)

    tr.forward_train, tr.update_average_meter = forward_train, update_average_meter
    start = [p.detach().clone() for p in tr.net.parameters()]
    tr.train(types.SimpleNamespace(selection_iter=1, get_trainset=lambda: _Train()))
    assert seen['lowres'] == [True, True]
    for m in seen['meters']:
        assert set(m) == {'train-loss', 'pos-loss', 'group-loss'} and all(bool(torch.isfinite(v)) for v in m.values())
        assert float(m['group-loss']) > 0 and float(m['pos-loss']) > 0
    grads = [p.grad for p in tr.net.parameters() if p.grad is not None]
    assert grads and any(float(g.abs().max()) > 0 for g in grads) and all(bool(torch.isfinite(g).all()) for g in grads)
    moved = sum(float((p.detach() - q).abs().sum()) for p, q in zip(tr.net.parameters(), start))
    assert moved > 0 and np.isfinite(moved)

"""The cross-view hierarchical group terms on the GPU: the weak-view tables (group scan, k_hier_pairs, k_hier_weights) and the strong-view
sums (k_hier_fwd / _bwd, k_whier_fwd / _bwd of csrc/online_plbl.hip) against the library's host loop through csrc/hier_group.h
(``ops.async_hier_loss_reference``) bit for bit, the module forms against the executed reference (tests/golden/g20_async_hier.npz),
``forward_lowres`` against the materialised upsample, run-to-run identical bytes, the map-only augmentation entry, the two-view loader
and both trainers end to end."""
import gc
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
from test_async_hier_cpu import GOLDEN, KEYS, views
from test_hier_group_cpu import bits_of, small_map, with_last_column
from test_losses_gpu import _inputs

pytestmark = pytest.mark.gpu
# strong (N, C, h, w, H, W), weak (h_o, w_o, H_o, W_o), S, Ss: the golden maps at quarter resolution with both fine maps, a non-integer
# scale, a ragged two-tile row, and the generic class count
SHAPES = [((2, 20, 6, 8, 24, 32), (10, 11, 40, 44), 48, 12), ((2, 20, 6, 8, 24, 32), (10, 11, 40, 44), 48, 192),
          ((2, 21, 9, 10, 33, 37), (12, 15, 45, 58), 150, 40), ((1, 19, 3, 75, 9, 300), (5, 80, 17, 320), 24, 60),
          ((1, 7, 4, 4, 16, 16), (8, 8, 32, 32), 6, 9)]
_CASES = {}


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    return ops


def _nearest(n_in, n_out):
    return np.minimum((np.arange(n_out) + 0.5) * n_in / n_out, n_in - 1).astype(np.int64)


def _case(shape):
    """Host tensors of a shape, made once: a dict zw, spx_w, small_w, msk_w, bits (weak) and z, small, msk (strong).  The first two
    shapes take g20's maps; the others a nearest-resampled, flipped window of the weak maps whose last columns are pad pixels (ids S
    and Ss), two of them with the mask byte set."""
    if shape not in _CASES:
        (N, C, h, w, H, W), (ho, wo, Ho, Wo), S, Ss = shape
        if (Ho, Wo, S) == (40, 44, 48):
            v = views(Ss)
            spx_w, small_w, msk_w, tgt = v['spx_w'], v['small_w'], v['msk_w'], v['tgt'][..., :-1]
            small, msk = v['small'], v['msk']
        else:
            seed = 700 + Wo + C
            _, tgt, spx_w, msk_w = _inputs(seed, N, C, Ho, Wo, S)
            small_w = small_map(seed, spx_w, S, Ss)
            ys, xs = 1 + _nearest(Ho - 3, H), 2 + _nearest(Wo - 5, W)
            small = np.ascontiguousarray(small_w[:, ys][:, :, xs][:, :, ::-1])
            msk = np.ascontiguousarray(msk_w[:, ys][:, :, xs][:, :, ::-1])
            small[:, :, -3:] = Ss
            msk[:, :, -3:] = False
            msk[:, :2, -1] = True
        _CASES[shape] = dict(zw=torch.from_numpy(synth.logits(31 + ho, N, C, ho, wo)), spx_w=torch.from_numpy(spx_w),
                             small_w=torch.from_numpy(small_w), msk_w=torch.from_numpy(msk_w), bits=bits_of(tgt),
                             z=torch.from_numpy(synth.logits(77 + h, N, C, h, w)), small=torch.from_numpy(small), msk=torch.from_numpy(msk))
    return _CASES[shape]


def _equal_to_the_reference(ops, c, size, size_w, Ss, weight, dtypes=(torch.int64,)):
    grad = torch.tensor([16.0], dtype=torch.float32)
    ref = ops.async_hier_loss_reference(c['z'], size, c['small'], Ss, c['msk'], weak=(c['zw'], size_w, c['spx_w'], c['small_w'], c['msk_w'], c['bits']),
                                        weight_reduce=weight, grad=grad)
    assert int(ref['acc'][1]) > 0 and bool(ref['dzq_fix'].any())
    zg, zwg, mg, mwg, bg, gg = c['z'].cuda(), c['zw'].cuda(), c['msk'].cuda(), c['msk_w'].cuda(), c['bits'].cuda(), grad.cuda()
    for dt in dtypes:
        what = (tuple(c['z'].shape), size, size_w, Ss, weight, dt)
        tab = ops.async_hier_tables(zwg, size_w, c['spx_w'].to(dt).cuda(), c['small_w'].to(dt).cuda(), Ss, mwg, bg, weight_reduce=weight)
        assert torch.equal(tab['gmax'].cpu(), ref['gmax']), what
        assert torch.equal(tab['mult'].cpu(), ref['mult']) and torch.equal(tab['any'].cpu(), ref['any']), what
        if weight is None:
            assert tab['wgt'] is None
        else:
            assert torch.equal(tab['wgt'].cpu().view(torch.int32), ref['wgt'].view(torch.int32)), what
            assert bool((tab['wgt'][tab['mult'] > 0] > 0).all()) and not bool(tab['wgt'][tab['mult'] == 0].any())
        fg = c['small'].to(dt).cuda()
        loss, acc = ops.async_hier_loss_fwd(zg, size, fg, Ss, mg, tab['mult'], tab['any'], tab['wgt'])
        assert torch.equal(acc.cpu(), ref['acc']), what
        assert torch.equal(loss.cpu().view(torch.int32), ref['loss'].view(torch.int32)), what
        dz, fix = ops.async_hier_loss_bwd(zg, size, fg, Ss, mg, tab['mult'], tab['any'], tab['wgt'], acc, gg, want_fix=True)
        assert torch.equal(fix.cpu(), ref['dzq_fix']), what
        assert torch.equal(dz.cpu().view(torch.int32), ref['dz'].view(torch.int32)), what
    return ref


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("weight", [None, 'max', 'mean'])
def test_kernels_equal_the_host_reference_bit_for_bit(shape, weight):
    ops = _gpu()
    (N, C, h, w, H, W), (ho, wo, Ho, Wo), S, Ss = shape
    _equal_to_the_reference(ops, _case(shape), (H, W), (Ho, Wo), Ss, weight, (torch.int64, torch.int32))


def test_the_weighted_count_differs_from_the_unweighted_one_only_through_zero_weights():
    """A table of the caller's own: pairs whose weight is set to 0 leave sum, count and gradient, on the device as on the host."""
    ops = _gpu()
    shape = SHAPES[0]
    (N, C, h, w, H, W), (ho, wo, Ho, Wo), S, Ss = shape
    c = _case(shape)
    tab = ops.async_hier_tables(c['zw'].cuda(), (Ho, Wo), c['spx_w'].cuda(), c['small_w'].cuda(), Ss, c['msk_w'].cuda(), c['bits'].cuda(),
                                weight_reduce='max')
    wgt = tab['wgt'].clone()
    pairs = torch.nonzero(tab['mult'] > 0)[::2]
    wgt[pairs[:, 0], pairs[:, 1], pairs[:, 2]] = 0.0
    grad = torch.tensor([16.0], dtype=torch.float32)
    zg, fg, mg = c['z'].cuda(), c['small'].cuda(), c['msk'].cuda()
    loss, acc = ops.async_hier_loss_fwd(zg, (H, W), fg, Ss, mg, tab['mult'], tab['any'], wgt)
    _, full = ops.async_hier_loss_fwd(zg, (H, W), fg, Ss, mg, tab['mult'], tab['any'], tab['wgt'])
    dz, fix = ops.async_hier_loss_bwd(zg, (H, W), fg, Ss, mg, tab['mult'], tab['any'], wgt, acc, grad.cuda(), want_fix=True)
    ref = ops.async_hier_loss_reference(c['z'], (H, W), c['small'], Ss, c['msk'], tables=(tab['mult'].cpu(), tab['any'].cpu(), wgt.cpu()), grad=grad)
    assert 0 < int(acc[1]) < int(full[1])
    assert torch.equal(acc.cpu(), ref['acc']) and torch.equal(fix.cpu(), ref['dzq_fix'])
    assert torch.equal(loss.cpu().view(torch.int32), ref['loss'].view(torch.int32))


@pytest.mark.parametrize("Ss", [192, 12])
@pytest.mark.parametrize("key", list(KEYS))
def test_the_full_resolution_modules_match_the_reference_and_the_golden(Ss, key):
    """h = H, w = W in both views: the taps are exactly (1, 0).  Bit for bit against the host loop; the modules, called with the
    reference's signature, against the executed reference at the tolerance of tests/test_async_hier_cpu.py (1e-4 * max(1, |ref|) for the
    loss, 1e-4 * max|ref| for the gradient, the count exactly)."""
    ops = _gpu()
    from mulactseg_amd.utils import loss as L
    g = np.load(GOLDEN)
    v = views(Ss)
    k = "%s_%d" % (key, Ss)
    t = {n: torch.from_numpy(a) for n, a in v.items()}
    c = dict(zw=t['zw'], spx_w=t['spx_w'], small_w=t['small_w'], msk_w=t['msk_w'], bits=bits_of(v['tgt'][..., :-1]), z=t['z'], small=t['small'],
             msk=t['msk'])
    _equal_to_the_reference(ops, c, None, None, Ss, KEYS[key])
    args = types.SimpleNamespace(small_nseg=Ss)
    C, S = v['z'].shape[1], v['tgt'].shape[1]

    def crit(reduction):
        if KEYS[key] is None:
            return L.AsyncHierGroupMultiLabelCE(args, C, S, False, -1, reduction=reduction, temperature=0.1)
        return L.WeightAsyncHierGroupMultiLabelCE(args, C, S, False, -1, reduction=reduction, temperature=0.1, weight_reduce=KEYS[key])
    d = {n: a.cuda() for n, a in t.items()}
    before = d['tgt'].clone()
    zg = d['z'].clone().requires_grad_(True)
    m = crit('mean')
    loss = m(zg, d['zw'], d['tgt'], d['msk'], d['msk_w'], d['spx'], d['spx_w'], d['small'], d['small_w'])
    (float(g['weight']) * loss).backward()
    ref, gref = float(g[k + '_loss']), g[k + '_grad']
    err, scale = float(np.max(np.abs(zg.grad.cpu().numpy() - gref))), float(np.max(np.abs(gref)))
    print("g20 %s: loss %.7g golden %.7g, n %d golden %d, gradient error %.3e of %.3e" % (k, float(loss), ref, int(m.last_acc[1]), int(g[k + '_n']),
                                                                                         err, scale))
    assert int(m.last_acc[1]) == int(g[k + '_n'])
    assert abs(float(loss) - ref) <= 1e-4 * max(1.0, abs(ref))
    assert scale > 0 and err <= 1e-4 * scale
    assert torch.equal(d['tgt'], before)
    s, n1 = crit('none')(d['z'], d['zw'], d['tgt'], d['msk'], d['msk_w'], d['spx'], d['spx_w'], d['small'], d['small_w'])
    assert int(n1) == int(g[k + '_n']) + 1 and abs(float(s) - float(g[k + '_sum'])) <= 1e-4 * max(1.0, abs(float(g[k + '_sum'])))


@pytest.mark.parametrize("weight", [None, 'max', 'mean'])
def test_forward_lowres_equals_the_materialised_upsample(weight):
    ops = _gpu()
    from mulactseg_amd.utils import loss as L
    shape = SHAPES[2]
    (N, C, h, w, H, W), (ho, wo, Ho, Wo), S, Ss = shape
    c = {k: a.cuda() for k, a in _case(shape).items()}
    low = ops.async_hier_tables(c['zw'], (Ho, Wo), c['spx_w'], c['small_w'], Ss, c['msk_w'], c['bits'], weight_reduce=weight)
    full = ops.async_hier_tables(ops.upsample_bilinear(c['zw'], (Ho, Wo)), None, c['spx_w'], c['small_w'], Ss, c['msk_w'], c['bits'],
                                 weight_reduce=weight)
    for k in ('gmax', 'mult', 'any') + (() if weight is None else ('wgt',)):
        assert torch.equal(low[k].view(torch.uint8), full[k].view(torch.uint8)), k
    l0, a0 = ops.async_hier_loss_fwd(c['z'], (H, W), c['small'], Ss, c['msk'], low['mult'], low['any'], low['wgt'])
    l1, a1 = ops.async_hier_loss_fwd(ops.upsample_bilinear(c['z'], (H, W)), None, c['small'], Ss, c['msk'], low['mult'], low['any'], low['wgt'])
    assert int(a0[1]) > 0 and torch.equal(a0, a1) and torch.equal(l0.view(torch.int32), l1.view(torch.int32))
    # the module forms: forward_lowres against forward on the materialised logits of both views
    tgt = torch.zeros((N, S, C + 1), dtype=torch.uint8, device='cuda')
    for b in range(C):
        tgt[..., b] = ((c['bits'] >> b) & 1).to(torch.uint8)
    args = types.SimpleNamespace(small_nseg=Ss)
    m = (L.AsyncHierGroupMultiLabelCE(args, C, S, False, -1) if weight is None
         else L.WeightAsyncHierGroupMultiLabelCE(args, C, S, False, -1, weight_reduce=weight))
    spx = torch.zeros_like(c['small'])
    a = m.forward_lowres(c['z'], (H, W), c['zw'], (Ho, Wo), tgt, c['msk'], c['msk_w'], spx, c['spx_w'], c['small'], c['small_w'])
    acc_a = m.last_acc.clone()
    b = m(ops.upsample_bilinear(c['z'], (H, W)), ops.upsample_bilinear(c['zw'], (Ho, Wo)), tgt, c['msk'], c['msk_w'], spx, c['spx_w'], c['small'],
          c['small_w'])
    assert torch.equal(acc_a, m.last_acc) and torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(acc_a, a0)


def test_two_launches_leave_identical_bytes():
    ops = _gpu()
    shape = SHAPES[0]
    (N, C, h, w, H, W), (ho, wo, Ho, Wo), S, Ss = shape
    c = {k: a.cuda() for k, a in _case(shape).items()}
    gg = torch.tensor([16.0], dtype=torch.float32).cuda()
    for weight in (None, 'max', 'mean'):
        runs = []
        for _ in range(2):
            tab = ops.async_hier_tables(c['zw'], (Ho, Wo), c['spx_w'], c['small_w'], Ss, c['msk_w'], c['bits'], weight_reduce=weight)
            loss, acc = ops.async_hier_loss_fwd(c['z'], (H, W), c['small'], Ss, c['msk'], tab['mult'], tab['any'], tab['wgt'])
            dz, fix = ops.async_hier_loss_bwd(c['z'], (H, W), c['small'], Ss, c['msk'], tab['mult'], tab['any'], tab['wgt'], acc, gg, want_fix=True)
            runs.append([tab[k].clone() for k in ('gmax', 'mult', 'any')] + ([] if weight is None else [tab['wgt'].clone()]) + [loss, acc, dz, fix])
        for a, b in zip(*runs):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_forward_lowres_builds_no_full_resolution_tensor():
    _gpu()
    from mulactseg_amd.utils import loss as L
    N, C, h, w, H, W, ho, wo, Ho, Wo, S, Ss = 2, 19, 48, 48, 192, 192, 64, 96, 256, 384, 64, 256
    _, tgt, spx_w, msk_w = _inputs(5, N, C, Ho, Wo, S)
    small_w = small_map(5, spx_w, S, Ss)
    crit = L.WeightAsyncHierGroupMultiLabelCE(types.SimpleNamespace(small_nseg=Ss), C, S, False, -1, weight_reduce='mean')
    zq = torch.from_numpy(synth.logits(6, N, C, h, w)).cuda().requires_grad_(True)
    zw = torch.from_numpy(synth.logits(7, N, C, ho, wo)).cuda()
    tg = torch.from_numpy(with_last_column(tgt)).cuda()
    sw, fw, mw = (torch.from_numpy(a).cuda() for a in (spx_w, small_w, msk_w))
    sp, sm, mk = (a[:, 32:32 + H, 100:100 + W].contiguous() for a in (sw, fw, mw))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    group = crit.forward_lowres(zq, (H, W), zw, (Ho, Wo), tg, mk, mw, sp, sw, sm, fw)
    pos = crit.merged_positive(zq, (H, W), sp, mk, 0.1)
    (16.0 * pos + group).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("peak allocation of a forward_lowres step: %d bytes; one strong [N,C,H,W] f32 tensor: %d bytes" % (peak, N * C * H * W * 4))
    assert peak < N * C * H * W * 4 and float(group) > 0 and float(zq.grad.abs().max()) > 0


def test_the_map_only_entry_writes_what_the_two_map_kernel_writes():
    _gpu()
    from mulactseg_amd.dataloader.device_transforms import DeviceResize, DeviceTrainAugment, DeviceTrainAugmentThreeMaps
    H, W, CROP = 96, 160, (128, 176)            # larger than the picture: the seeded draws below pad (scales 1.19 and 0.86) and flip
    rs = np.random.RandomState(3)
    img = torch.from_numpy(rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)).cuda()
    lab = torch.from_numpy(rs.randint(0, 34, size=(H, W)).astype(np.uint8)).cuda()
    spx = torch.from_numpy(synth.superpixel_map(1, H, W, 64).astype(np.int32)).cuda()
    fine = torch.from_numpy(synth.superpixel_map(2, H, W, 256).astype(np.int64)).cuda()
    three = DeviceTrainAugmentThreeMaps(pad_values=[0, 64, 256], size=CROP, rng=random.Random(9))
    two = DeviceTrainAugment(pad_values=[0, 64], size=CROP, rng=random.Random(9))
    third = DeviceTrainAugment(pad_values=[256], size=CROP)
    pads = flips = 0
    for _ in range(6):
        p = three._draw(H, W)
        assert p == two._draw(H, W)                                   # the same draws in the same order
        image, (a, b, c) = three(img, [lab, spx, fine], params=p)
        want_image, (wa, wb) = two(img, [lab, spx], params=p)
        _, (wc,) = third(img, [fine], params=p)
        assert torch.equal(image.view(torch.int32), want_image.view(torch.int32)) and torch.equal(a, wa) and torch.equal(b, wb)
        assert c.dtype == torch.int64 and torch.equal(c, wc)
        assert torch.equal(c == 256, b == 64)                          # one geometry: the pads coincide
        pads += int((c == 256).sum())
        flips += int(p['flip'])
    assert pads > 0 and 0 < flips < 6
    # the deterministic resize of the same three maps (the weak view)
    p, three.size = DeviceResize((2 * H, 2 * W)).geometry(H, W)
    image, (a, b, c) = three(img, [lab, spx, fine], params=p)
    want_image, (wa, wb) = DeviceResize((2 * H, 2 * W), pad_values=[0, 64])(img, [lab, spx])
    _, (wc,) = DeviceResize((2 * H, 2 * W), pad_values=[256])(img, [fine])
    assert tuple(c.shape) == (2 * H, 2 * W) and torch.equal(c, wc) and torch.equal(a, wa) and torch.equal(b, wb)
    assert torch.equal(image.view(torch.int32), want_image.view(torch.int32))
    with pytest.raises(ValueError):
        three(img, [lab, spx])


def test_the_loader_gives_two_consistent_views(tmp_path):
    """The stored fine map is 2 * spx + (x & 1) with small_nseg = 2 * nseg: in BOTH views small // 2 == spx whatever the geometry, pads
    included, and each mask is "selected" AND "training id != 255" of that view's own label picture."""
    _gpu()
    from mulactseg_amd import dataloader
    from mulactseg_amd.dataloader import region_cityscapes_or_tensor_ignore_async as mod
    dataloader.register_dataset_factory(None)
    H, W, NSEG, CROP = 96, 160, 64, 128
    tree = helpers.write_cityscapes_tree(str(tmp_path / 'data'), n=3, H=H, W=W, nseg=NSEG)
    fine_dir = os.path.join(tree['root'], 'superpixel_seed/cityscapes/seeds_%d/train/label' % (2 * NSEG))
    os.makedirs(fine_dir)
    for stem, spx in zip(tree['stems'], tree['spx']):
        fine = (2 * spx + (np.arange(W)[None, :] & 1)).astype(np.int32)
        with open(os.path.join(fine_dir, stem + '.pkl'), 'wb') as f:
            pickle.dump({'labels': fine, 'valid_idxes': np.unique(fine)}, f)
    flags = ['--method', 'active_joint_hier_multi_async', '--loader', 'region_cityscapes_or_tensor_ignore_async', '--train_transform',
             'rescale_769_multi_notrg_ignore', '--small_nseg', str(2 * NSEG)]
    with pytest.raises(NotImplementedError, match="load_smaller_spx"):
        dataloader.get_active_dataset(helpers.cityscapes_tree_args(tree, tmp_path / 'run0', flags), train_transform='rescale_769_multi_notrg_ignore')
    args = helpers.cityscapes_tree_args(tree, tmp_path / 'run', flags + ['--load_smaller_spx'])
    os.makedirs(args.model_save_dir, exist_ok=True)
    aset = dataloader.get_active_dataset(args, train_transform=args.train_transform)
    pool, label = aset.trg_pool_dataset, aset.trg_label_dataset
    assert type(label) is mod.RegionCityscapesOr and label.transform.n_maps == 3 and label.transform.all_pad_values == [0, NSEG, 2 * NSEG]
    label.transform.size = (CROP, CROP)
    assert label.weak_size == mod.WEAK_SIZE == (1024, 2048)
    label.weak_size = (2 * H, 2 * W)                                  # (smaller here to keep the test quick)
    assert set(pool[0]) == {'images', 'spx', 'labels'}                 # pool samples are the parent's
    aset.selection_iter = 1
    sel = [3, 7, 11, 40]
    aset.expand_training_set([(1.0 - 0.01 * i, ','.join(pool.im_idx[1]), s) for i, s in enumerate(sel)], 10 ** 6, 'x')
    files = label.sample_files(0)
    assert ('ids', label.small_spx_fname(label.im_idx[0][2])) in files and ('map', label.precise_label_file(label.im_idx[0][1])) in files
    label.transform.rng = random.Random(11)
    k = tree['stems'].index(label.im_idx[0][1].split('/')[-1].split('.')[0])
    tid, spx0 = tree['train_ids'][k], tree['spx'][k]
    weak_mask = np.isin(spx0, sel) & (tid != 255)
    assert weak_mask.any() and (np.isin(spx0, sel) & (tid == 255)).any()     # the ground truth does remove selected pixels
    ys, xs = _nearest(H, 2 * H), _nearest(W, 2 * W)
    pads = 0
    for _ in range(4):
        s = label[0]
        assert set(s) == {'images', 'image_weak', 'labels', 'spx', 'spx_weak', 'spmask', 'spmask_weak', 'spx_small', 'spx_small_weak', 'fnames'}
        assert tuple(s['images'].shape) == (3, CROP, CROP) and tuple(s['image_weak'].shape) == (3, 2 * H, 2 * W)
        for a, b, m, size in ((s['spx'], s['spx_small'], s['spmask'], (CROP, CROP)), (s['spx_weak'], s['spx_small_weak'], s['spmask_weak'], (2 * H, 2 * W))):
            assert tuple(a.shape) == tuple(b.shape) == tuple(m.shape) == size and a.is_cuda and m.dtype == torch.bool
            assert torch.equal(b // 2, a)
            selected = torch.from_numpy(np.isin(a.cpu().numpy(), sel))
            assert not bool((m.cpu() & ~selected).any()) and bool(m.any())
        # the weak view is the nearest resize of the stored maps: ids, and the mask from the stored ground truth
        assert np.array_equal(s['spx_weak'].cpu().numpy(), spx0[ys][:, xs])
        assert np.array_equal(s['spmask_weak'].cpu().numpy(), weak_mask[ys][:, xs])
        # the strong mask drops pixels of selected superpixels too (ignored ground truth), and never holds a pad pixel
        selected = torch.from_numpy(np.isin(s['spx'].cpu().numpy(), sel))
        assert bool((selected & ~s['spmask'].cpu()).any()) and not bool(s['spmask'][s['spx'] == NSEG].any())
        pads += int((s['spx'] == NSEG).sum())
        assert tuple(s['labels'].shape) == (NSEG, 20)
    assert pads > 0
    batch = dataloader.collate_fn([label[0], label[0]])
    assert tuple(batch['image_weak'].shape) == (2, 3, 2 * H, 2 * W) and tuple(batch['spx_small_weak'].shape) == (2, 2 * H, 2 * W)


class _Train(torch.utils.data.Dataset):
    """Two samples: a 128 x 128 crop (flipped) of a 160 x 192 weak view, with a fine map of 256 ids."""
    H = W = 128
    HO, WO = 160, 192
    S, Ss, cols = 64, 256, 20

    def __init__(self):
        self.selection_iter = 1

    def __len__(self):
        return 2

    def __getitem__(self, i):
        rs = np.random.RandomState(100 + i)
        spx, msk = synth.train_crop(200 + i, self.HO, self.WO, self.S, frac_selected=0.3)
        small = small_map(400 + i, spx[None], self.S, self.Ss)[0]

        def crop(a):
            return torch.from_numpy(np.ascontiguousarray(a[16:16 + self.H, 40:40 + self.W][:, ::-1]))
        return {'images': torch.from_numpy(rs.standard_normal((3, self.H, self.W)).astype(np.float32)),
                'image_weak': torch.from_numpy(rs.standard_normal((3, self.HO, self.WO)).astype(np.float32)),
                'labels': torch.from_numpy(synth.multi_hot_targets(300 + i, self.S, self.cols)),
                'spx': crop(spx), 'spmask': crop(msk), 'spx_small': crop(small),
                'spx_weak': torch.from_numpy(spx), 'spmask_weak': torch.from_numpy(msk), 'spx_small_weak': torch.from_numpy(small)}


class _Val(torch.utils.data.Dataset):
    def __len__(self):
        return 1

    def __getitem__(self, i):
        return {'images': torch.zeros((3, 128, 128)), 'labels': torch.zeros((128, 128), dtype=torch.int64)}


@pytest.mark.parametrize("method,extra,freeze", [('active_joint_hier_multi_async', [], False), ('active_joint_hier_multi_async_weight', [], False),
                                                 ('active_joint_hier_multi_async_weight', ['--weight_reduce', 'mean'], True)])
def test_the_trainers_run_a_quarter_resolution_step(method, extra, freeze):
    _gpu()
    import importlib
    from mulactseg_amd import dataloader
    from mulactseg_amd.utils import common, loss as L
    a = common.get_parser().parse_args([
        '-m', 'deeplabv3pluswn_resnet50deepstem', '--separable_conv', '--method', method, '--ce_temp', '0.1', '--multi_ce_temp', '0.1',
        '--group_ce_temp', '0.1', '--coeff', '16.0', '--or_labeling', '--fair_counting', '--nseg', str(_Train.S), '--load_smaller_spx',
        '--small_nseg', str(_Train.Ss), '--train_batch_size', '2', '--val_batch_size', '1', '--num_workers', '0', '--val_num_workers', '0',
        '--train_lr', '2e-5', '--finetune_itrs', '2', '--val_period', '1000', '--log_period', '1', '-p', tempfile.mkdtemp()] + extra)
    a.pretrained_backbone = False
    a.lowres_loss = True
    a.freeze_bn = freeze
    dataloader.register_dataset_factory(lambda args, name, data_root, datalist, imageset: _Val())
    torch.manual_seed(0)
    tr = importlib.import_module("mulactseg_amd.trainer." + method).ActiveTrainer(a, logging.getLogger("test"), 1)
    tr._wandb_log = lambda payload, step: None
    weighted = method.endswith('weight')
    assert type(tr.hier_group_multi_loss) is (L.WeightAsyncHierGroupMultiLabelCE if weighted else L.AsyncHierGroupMultiLabelCE)
    if weighted:
        assert tr.hier_group_multi_loss.weight_reduce == ('mean' if extra else 'max')
    seen = dict(train=[], teacher=[], meters=[])
    fwd, meter_fn, net_fwd = tr.forward_train, tr.update_average_meter, tr.net.forward
    bns = [m for m in tr.net.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]

    def forward_train(images, **kw):
        out = fwd(images, **kw)
        seen['train'].append((kw.get('lowres', False), tuple(out.shape), tr.net.training, torch.is_grad_enabled()))
        return out

    def net_forward(images, *args, **kw):
        if not torch.is_grad_enabled():             # the teacher forward: eval mode everywhere, on the weak view
            seen['teacher'].append((tuple(images.shape[-2:]), tr.net.training, any(m.training for m in bns), kw.get('lowres', False)))
        return net_fwd(images, *args, **kw)

    def update_average_meter(values):
        seen['meters'].append({k: v.detach().clone() for k, v in values.items()})
        seen['modes'] = (tr.net.training, [m.training for m in bns])
        return meter_fn(values)

    tr.forward_train, tr.update_average_meter, tr.net.forward = forward_train, update_average_meter, net_forward
    start = [p.detach().clone() for p in tr.net.parameters()]
    try:
        tr.train(types.SimpleNamespace(selection_iter=1, get_trainset=lambda: _Train()))
    finally:            # the hooks above close a cycle through the trainer: break it, so the model dies here and not in a later test
        del tr.forward_train, tr.update_average_meter, tr.net.forward
    assert seen['train'] == [(True, (2, 19, 32, 32), True, True)] * 2
    assert seen['teacher'] == [((_Train.HO, _Train.WO), False, False, True)] * 2
    # every module is back in the mode it had: the net trains, and a BatchNorm frozen by --freeze_bn stays frozen
    assert seen['modes'][0] is True and bns and all(m is (not freeze) for m in seen['modes'][1])
    for m in seen['meters']:
        assert set(m) == {'train-loss', 'pos-loss', 'group-loss'} and all(bool(torch.isfinite(v)) for v in m.values())
        assert float(m['group-loss']) > 0 and float(m['pos-loss']) > 0
    assert int(tr.hier_group_multi_loss.last_acc[1]) > 0
    grads = [p.grad for p in tr.net.parameters() if p.grad is not None]
    assert grads and any(float(g.abs().max()) > 0 for g in grads) and all(bool(torch.isfinite(g).all()) for g in grads)
    moved = sum(float((p.detach() - q).abs().sum()) for p, q in zip(tr.net.parameters(), start))
    assert moved > 0 and np.isfinite(moved)
    del tr, grads, bns, fwd, meter_fn, net_fwd
    gc.collect()

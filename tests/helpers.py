"""Test helpers: an oracle-backed stand-in for the HIP backend (CPU tests of the host logic only) and
tiny fake trainer / pool objects shaped like the reference's plugin arguments."""
import types

import numpy as np
import torch

from oracle import exact, port


class OracleBackend:
    """Implements the backend protocol of mulactseg_amd.active_selection.engine with the CPU oracle.
    TEST INFRASTRUCTURE: lives under tests/, is never importable from the product package."""
    name = "oracle"

    def __init__(self):
        self.device = torch.device('cpu')

    def inv_temperature(self, T):
        return float(exact.inv_temperature(T))

    def class_prob_sum(self, logits, invT, out):
        out += torch.from_numpy(exact.class_prob_sum(logits.numpy(), np.float32(invT)).view(np.int64))

    def region_accum(self, logits, spx, cls_w, S, invT, score_sum, hist):
        s, h = exact.bvsb_region_accum(logits.numpy(), spx.numpy(), None if cls_w is None else cls_w.numpy(), S,
                                       np.float32(invT))
        score_sum += torch.from_numpy(s.view(np.int64))
        hist += torch.from_numpy(h.view(np.int32))

    def finalize(self, score_sum, hist, ban_class, want_hist_i64=False):
        score, dom, cnt = exact.region_finalize(score_sum.numpy().view(np.uint64), hist.numpy().view(np.uint32), ban_class)
        h64 = hist.to(torch.int64) if want_hist_i64 else None
        return torch.from_numpy(score), torch.from_numpy(dom), torch.from_numpy(cnt.view(np.int32)), h64

    def single_pass(self, logits, spx, S, invT, prob_sum, class_sum, hist):
        ps, cs, h = exact.single_pass_accum(logits.numpy(), spx.numpy(), S, np.float32(invT))
        prob_sum += torch.from_numpy(ps.view(np.int64))
        class_sum += torch.from_numpy(cs.view(np.int64))
        hist += torch.from_numpy(h.view(np.int32))

    def single_pass_lowres(self, zq, size, spx, S, invT, prob_sum, class_sum, hist):
        full = exact.upsample_bilinear(zq.numpy(), int(size[0]), int(size[1]))
        self.single_pass(torch.from_numpy(full), spx, S, invT, prob_sum, class_sum, hist)

    def class_weight(self, prob_sum, hw, batch_size, n_batches, coeff):
        from mulactseg_amd.active_selection.engine import class_weight_from_sums
        n_img = prob_sum.shape[0]
        cum, w = class_weight_from_sums(prob_sum.numpy(), hw, np.arange(n_img) // batch_size, n_batches, coeff)
        return cum, torch.from_numpy(w)

    def finalize_weighted(self, class_sum, hist, cls_w, ban_class, want_hist_i64=False):
        w = np.ones(hist.shape[-1], dtype=np.float32) if cls_w is None else cls_w.numpy()
        score, dom, cnt = exact.region_finalize_weighted(class_sum.numpy().view(np.uint64), hist.numpy().view(np.uint32),
                                                         exact.weights_to_fixed31(w), ban_class)
        h64 = hist.to(torch.int64) if want_hist_i64 else None
        return torch.from_numpy(score), torch.from_numpy(dom), torch.from_numpy(cnt.view(np.int32)), h64

    def minmax_normalize_(self, scores):
        u = scores.numpy()
        mn = u[u != 0].min()
        u -= mn
        u /= u.max()
        return scores

    def region_reweight_(self, scores, dominant, ban_class, cls_w):
        s, d = scores.numpy(), dominant.numpy()
        s[d == ban_class] = 0
        if cls_w is not None:
            s *= cls_w.numpy()[d]
        return scores

    def dominant_hist(self, dominant, C):
        return torch.from_numpy(np.bincount(dominant.numpy().ravel(), minlength=C).astype(np.int64))

    def select(self, scores, valid, img_rank, img_of_rank, region_cost, budget, max_out):
        # reference semantics: Python tuple sort with the rank standing in for the path string
        s = scores.numpy()
        v = np.ones(s.shape, dtype=bool) if valid is None else valid.numpy()        # (None: every region is still in the pool)
        rank = img_rank.numpy()
        tuples = [(float(s[i, r]), int(rank[i]), r) for i in range(s.shape[0]) for r in range(s.shape[1]) if v[i, r]]
        inv = img_of_rank.numpy()
        cost = None if region_cost is None else region_cost.numpy()
        fn = None if cost is None else (lambda rk, rid: int(cost[inv[rk], rid]))
        taken = port.select_regions(tuples, budget, fn)
        return (len(taken), np.array([inv[t[1]] for t in taken], dtype=np.int32),
                np.array([t[2] for t in taken], dtype=np.int32), np.array([t[0] for t in taken], dtype=np.float32))


    def select_sharded(self, plan, scores, valid, img_rank, img_of_rank, region_cost, budget, max_out):
        """The sharded K4 of engine.select_regions restated on tuples: local head of max_out regions, all-gather, merged walk."""
        import torch.distributed as dist
        s = scores.numpy()
        v = np.ones(s.shape, dtype=bool) if valid is None else valid.numpy()
        rank = img_rank.numpy()
        local = sorted(((float(s[i, r]), int(rank[i]), r) for i in range(plan.img_lo, plan.img_hi) for r in range(s.shape[1]) if v[i, r]),
                       reverse=True)[:max_out]
        heads = [None] * plan.world
        dist.all_gather_object(heads, local)
        merged = sorted((t for h in heads for t in h), reverse=True)
        inv = img_of_rank.numpy()
        cost = None if region_cost is None else region_cost.numpy()
        fn = None if cost is None else (lambda rk, rid: int(cost[inv[rk], rid]))
        taken = port.select_regions(merged, budget, fn)
        return (len(taken), np.array([inv[t[1]] for t in taken], dtype=np.int32),
                np.array([t[2] for t in taken], dtype=np.int32), np.array([t[0] for t in taken], dtype=np.float32))


class FakePool(torch.utils.data.Dataset):
    """Pool dataset whose 'images' ARE the logits (the fake trainer's net is the identity)."""

    def __init__(self, logits, spx, im_idx, suppix):
        self.logits, self.spx = torch.from_numpy(logits), torch.from_numpy(spx)
        self.im_idx = [list(k) for k in im_idx]
        self.suppix = {k: list(v) for k, v in suppix.items()}

    def __len__(self):
        return len(self.im_idx)

    def __getitem__(self, i):
        return {'images': self.logits[i], 'spx': self.spx[i]}


def fake_trainer(device='cpu', save_dir=None):
    return types.SimpleNamespace(net=torch.nn.Identity(), device=torch.device(device), model_save_dir=save_dir,
                                 selection_iter=1)


def selector_args(**kw):
    base = dict(val_batch_size=2, val_num_workers=0, nseg=64, active_method='x', num_classes=19, ce_temp=0.1,
                cls_weight_coeff=6.0, method='active_joint_multi_predignore_lossdecomp', save_scores=False,
                fair_counting=True, or_labeling=True, model_save_dir=None, finetune_itrs=1,
                wandb=types.SimpleNamespace(log=lambda *a, **k: None))
    base.update(kw)
    return types.SimpleNamespace(**base)


class OracleLossOps:
    """CPU stand-in for the part of mulactseg_amd.ops the loss modules call (partial_loss_fwd_fused / _bwd_fused, LossState,
    inv_temperature), backed by oracle/exact.c -- lets the world-size-2 gloo tests drive FusedPartialLabelLoss's normaliser
    all-reduce and autograd wiring without a GPU.  Full-resolution logits only.  TEST INFRASTRUCTURE."""

    class LossState:
        pass

    @staticmethod
    def inv_temperature(T):
        return float(exact.inv_temperature(T))

    @staticmethod
    def partial_loss_fwd_fused(z, size, spx, mask, invT, flags, targets=None, cols_used=None, bits=None, weights=None, reduce_acc=None):
        import ctypes
        assert size is None and weights is None
        if bits is None:
            bits = torch.from_numpy(exact.target_bits(targets.numpy(), cols_used).view(np.int32))
        acc, gmax, _ = exact.partial_loss_fwd(z.detach().numpy(), spx.numpy(), mask.numpy().astype(np.uint8), bits.numpy().view(np.uint32),
                                              np.float32(invT), flags)
        acc_t = torch.from_numpy(acc.view(np.int64).copy())
        if reduce_acc is not None:
            reduce_acc(acc_t)                            # the all-reduce of the integer sums and counts under test
        accn = np.ascontiguousarray(acc_t.numpy().view(np.uint64))
        losses = np.zeros(3, dtype=np.float32)
        exact.lib().exact_loss_values(accn.ctypes.data_as(ctypes.c_void_p), flags, losses.ctypes.data_as(ctypes.c_void_p))
        st = OracleLossOps.LossState()
        st.acc, st.flags = acc_t, flags
        st.N, st.S, st.C = z.shape[0], bits.shape[1], z.shape[1]
        st.bits = bits
        # (what the product keeps in its work buffer: acc | table | bit masks)
        st.work = torch.cat([acc_t, torch.from_numpy(gmax.view(np.int64)).reshape(-1), bits.reshape(-1).to(torch.int64)])
        return torch.from_numpy(losses), st

    @staticmethod
    def partial_loss_bwd_fused(z, size, spx, mask, state, grad, invT, weights=None, want_fix=False):
        assert size is None and weights is None
        n_tab = state.N * state.S * state.C
        acc = state.work[:8]
        gmax = state.work[8:8 + n_tab].reshape(state.N, state.S, state.C)
        bits = state.work[8 + n_tab:].to(torch.int32).reshape(state.N, state.S)
        _, dz = exact.partial_loss_bwd(z.detach().numpy(), spx.numpy(), mask.numpy().astype(np.uint8), bits.numpy().view(np.uint32),
                                       gmax.numpy().view(np.uint64), acc.numpy().view(np.uint64), grad.numpy(), np.float32(invT), state.flags)
        return torch.from_numpy(dz)


# ---- test-support library (tests/libmulactseg_test.so, built from mulactseg_amd/csrc/test_support.hip by build()) --------------
_TEST_LIB = None


def _test_lib():
    """TEST INFRASTRUCTURE: the CU-hogging neighbour kernel lives in its own library, not in the product ABI."""
    global _TEST_LIB
    if _TEST_LIB is None:
        import ctypes
        import os
        from mulactseg_amd import _lib
        _lib.load()                                  # (torch's HIP runtime first: one runtime per process)
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libmulactseg_test.so")
        if not os.path.exists(path):
            raise RuntimeError("%s is not built: run `make -C mulactseg_amd/csrc`" % path)
        lib = ctypes.CDLL(path)
        lib.mas_test_occupy.restype = ctypes.c_int
        lib.mas_test_occupy.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_void_p]
        _TEST_LIB = lib
    return _TEST_LIB


def occupy_cus(blocks, lds_bytes, seconds, stream=None):
    """`blocks` workgroups that hold 256 threads + `lds_bytes` of LDS for `seconds` (bounded: every wave leaves after that)."""
    from mulactseg_amd import _lib
    st = torch.cuda.current_stream() if stream is None else stream
    _lib.check(_test_lib().mas_test_occupy(int(blocks), int(lds_bytes), int(seconds * 1e8), st.cuda_stream), "mas_test_occupy")


# ---------------------------------------------------------------------------------------------------------------------------
# a tiny Cityscapes-shaped directory tree in the reference's on-disk formats
# ---------------------------------------------------------------------------------------------------------------------------
CITY_TRAIN_IDS = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]     # raw ids of the 19 training classes


def write_cityscapes_tree(root, n=5, H=128, W=256, nseg=64, n_val=2, seed=0, trim=5):
    """Writes pictures (``leftImg8bit/train/<city>/*_leftImg8bit.png``), raw label PNGs (``gtFine/train/<city>/*_gtFine_labelIds.png``),
    superpixel pickles (``superpixel_seed/cityscapes/seeds_<nseg>/train/label/*.pkl`` = ``{'labels': int32 [H,W], 'valid_idxes': ...}``),
    the multi-hot tensor + sizes (``.../gtFine_multi_tensor_trim_<k>x<k>/{multi_hot_cls,sp_size}.npy``), the target datalist
    (``train_seed<nseg>_or.txt``: picture, ``gtFine_or/<stem>.npy``, superpixel file -- tab separated), the region dictionary
    (``{spx path: [nseg, [missing ids]]}``) and a validation list (``val.txt``, whitespace separated, labelIds PNGs).
    Returns a dict of the paths and the arrays that were written."""
    import json
    import os
    import pickle
    from PIL import Image
    from mulactseg_amd import synth
    rs = np.random.RandomState(seed)
    cities = ['aachen', 'bochum']
    out = {'root': str(root), 'pictures': [], 'raw_labels': [], 'train_ids': [], 'spx': [], 'stems': [], 'H': H, 'W': W, 'nseg': nseg, 'val_lines': []}
    spx_dir = os.path.join(root, 'superpixel_seed/cityscapes/seeds_%d/train' % nseg)
    os.makedirs(os.path.join(spx_dir, 'label'), exist_ok=True)
    mt_dir = os.path.join(spx_dir, 'gtFine_multi_tensor_trim_%dx%d' % (trim, trim))
    os.makedirs(mt_dir, exist_ok=True)
    lines, region = [], {}
    multi_hot = np.zeros((n, nseg, 20), dtype=np.uint8)
    sizes = np.zeros((n, nseg), dtype=np.int32)
    lut = np.full(256, 255, dtype=np.int64)
    lut[CITY_TRAIN_IDS] = np.arange(19)
    for k in range(n + n_val):
        split = 'train' if k < n else 'val'
        city = cities[k % 2]
        stem = '%s_%06d_000019' % (city, k)
        cls = synth.class_map(seed * 1000 + k, H, W, 19, blob=16)                       # training ids 0..18
        raw = np.asarray(CITY_TRAIN_IDS, dtype=np.uint8)[cls]
        raw[rs.uniform(size=raw.shape) < 0.04] = 3                                       # some "out of roi" pixels -> ignored (255)
        pic = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
        for sub in ('leftImg8bit', 'gtFine'):
            os.makedirs(os.path.join(root, sub, split, city), exist_ok=True)
        img_rel = 'leftImg8bit/%s/%s/%s_leftImg8bit.png' % (split, city, stem)
        lbl_rel = 'gtFine/%s/%s/%s_gtFine_labelIds.png' % (split, city, stem)
        Image.fromarray(pic).save(os.path.join(root, img_rel))
        Image.fromarray(raw).save(os.path.join(root, lbl_rel))
        if split == 'val':
            out['val_lines'].append('%s %s %s' % (img_rel, lbl_rel, lbl_rel))
            continue
        spx = synth.superpixel_map(seed * 1000 + 500 + k, H, W, nseg).astype(np.int32)
        spx_rel = 'superpixel_seed/cityscapes/seeds_%d/train/label/%s.pkl' % (nseg, stem)
        with open(os.path.join(root, spx_rel), 'wb') as f:
            pickle.dump({'labels': spx, 'valid_idxes': np.unique(spx)}, f)
        tid = lut[raw]
        col = np.where(tid == 255, 19, tid)
        multi_hot[k, spx.reshape(-1), col.reshape(-1)] = 1
        sizes[k] = np.bincount(spx.reshape(-1), minlength=nseg)[:nseg]
        missing = sorted(set(range(nseg)) - set(np.unique(spx).tolist()))
        region[spx_rel] = [nseg, missing]
        lines.append('\t'.join([img_rel, 'superpixel_seed/cityscapes/seeds_%d/train/gtFine_or/%s.npy' % (nseg, stem), spx_rel]))
        out['pictures'].append(pic), out['raw_labels'].append(raw), out['train_ids'].append(tid), out['spx'].append(spx), out['stems'].append(stem)
    np.save(os.path.join(mt_dir, 'multi_hot_cls.npy'), multi_hot)
    np.save(os.path.join(mt_dir, 'sp_size.npy'), sizes)
    lists = os.path.join(root, 'lists')
    os.makedirs(lists, exist_ok=True)
    out['trg_datalist'] = os.path.join(lists, 'train_seed%d_or.txt' % nseg)
    out['region_dict'] = os.path.join(lists, 'train_seed%d.dict' % nseg)
    out['val_datalist'] = os.path.join(lists, 'val.txt')
    with open(out['trg_datalist'], 'w') as f:
        f.write('\n'.join(lines) + '\n')
    with open(out['region_dict'], 'w') as f:
        json.dump(region, f)
    with open(out['val_datalist'], 'w') as f:
        f.write('\n'.join(out['val_lines']) + '\n')
    out['multi_hot'], out['sp_size'], out['lines'] = multi_hot, sizes, lines
    return out


def cityscapes_tree_args(tree, save_dir, extra=()):
    """The flags of the stage-1 production run (``script/open_source/train_city_mul_res50.sh``) pointed at ``tree``."""
    from mulactseg_amd.utils.common import get_parser
    a = get_parser().parse_args([
        '-m', 'deeplabv3pluswn_resnet50deepstem', '--separable_conv', '--method', 'active_joint_multi_predignore_lossdecomp',
        '--active_method', 'my_bvsb_predclsbal_pwr_banignore', '--cls_weight_coeff', '6.0', '--or_labeling', '--fair_counting',
        '--loss_type', 'joint_multi_loss', '--nseg', str(tree['nseg']), '--scheduler', 'poly', '--train_lr', '0.00002',
        '--train_transform', 'rescale_769_multi_notrg', '--loader', 'region_cityscapes_or_tensor', '--multi_ce_temp', '0.1',
        '--group_ce_temp', '0.1', '--ce_temp', '0.1', '--coeff', '16.0', '--coeff_mc', '8.0', '--coeff_gm', '1.0',
        '--trim_kernel_size', '5', '--trim_multihot_boundary', '--trg_data_dir', tree['root'], '--trg_datalist', tree['trg_datalist'],
        '--region_dict', tree['region_dict'], '--val_data_dir', tree['root'], '--val_datalist', tree['val_datalist'],
        '--train_batch_size', '2', '--val_batch_size', '2', '--num_workers', '0', '--val_num_workers', '0', '--finetune_itrs', '2',
        '--val_period', '2', '--log_period', '1', '--active_selection_size', '40', '-p', str(save_dir)] + list(extra))
    a.pretrained_backbone = False
    return a


def write_voc_tree(root, n=4, nseg=150, seed=0, trim=5, sizes=((120, 160), (150, 110), (96, 128), (130, 130))):
    """A tiny PASCAL-VOC-shaped tree in the reference's layout (dataloader/region_voc.py:75-84, region_voc_or_tensor.py:30-62):
    ``VOC2012/JPEGImages/<name>.jpg``, ``VOC2012/SegmentationClass/<name>.png`` (palette PNG of class indices, 255 = void),
    ``superpixels/pascal_voc_seg/seeds_32/train/label/<name>.pkl``, the multi-hot tensor with its "undefined" column
    (``.../gtFine_multi_tensor_trim_<k>x<k>/multi_hot_cls.npy`` u8 [n, nseg, 22]), a datalist of bare names and a region dictionary
    keyed by them.  Pictures have DIFFERENT sizes, as in VOC."""
    import json
    import os
    import pickle
    from PIL import Image
    from mulactseg_amd import synth
    rs = np.random.RandomState(seed)
    out = {'root': str(root), 'names': [], 'classes': [], 'spx': [], 'nseg': nseg}
    for d in ('VOC2012/JPEGImages', 'VOC2012/SegmentationClass', 'superpixels/pascal_voc_seg/seeds_32/train/label',
              'superpixels/pascal_voc_seg/seeds_32/train/gtFine_multi_tensor_trim_%dx%d' % (trim, trim), 'lists'):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    mh = np.zeros((n, nseg, 22), dtype=np.uint8)
    region = {}
    for k in range(n):
        H, W = sizes[k % len(sizes)]
        name = '2007_%06d' % (32 + 7 * k)
        cls = synth.class_map(seed * 100 + k, H, W, 21, blob=12).astype(np.uint8)
        cls[rs.uniform(size=cls.shape) < 0.05] = 255
        n_ids = 40 + 10 * k
        spx = (synth.superpixel_map(seed * 100 + 50 + k, H, W, n_ids) % n_ids).astype(np.int32)
        Image.fromarray(rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)).save(os.path.join(root, 'VOC2012/JPEGImages', name + '.jpg'), quality=95)
        pal = Image.fromarray(cls, mode='P')
        pal.putpalette([v for i in range(256) for v in ((i * 37) % 256, (i * 91) % 256, (i * 13) % 256)])
        pal.save(os.path.join(root, 'VOC2012/SegmentationClass', name + '.png'))
        with open(os.path.join(root, 'superpixels/pascal_voc_seg/seeds_32/train/label', name + '.pkl'), 'wb') as f:
            pickle.dump({'labels': spx}, f)
        col = np.where(cls == 255, 21, cls)
        mh[k, spx.reshape(-1), col.reshape(-1)] = 1
        region[name] = [int(spx.max()) + 1, sorted(set(range(int(spx.max()) + 1)) - set(np.unique(spx).tolist()))]
        out['names'].append(name), out['classes'].append(cls), out['spx'].append(spx)
    np.save(os.path.join(root, 'superpixels/pascal_voc_seg/seeds_32/train/gtFine_multi_tensor_trim_%dx%d' % (trim, trim), 'multi_hot_cls.npy'), mh)
    out['trg_datalist'] = os.path.join(root, 'lists', 'train_seed%d_or.txt' % nseg)
    out['region_dict'] = os.path.join(root, 'lists', 'train_seed%d.dict' % nseg)
    out['val_datalist'] = os.path.join(root, 'lists', 'val.txt')
    for path, names in ((out['trg_datalist'], out['names']), (out['val_datalist'], out['names'][:2])):
        with open(path, 'w') as f:
            f.write('\n'.join(names) + '\n')
    with open(out['region_dict'], 'w') as f:
        json.dump(region, f)
    out['multi_hot'] = mh
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# float32 rounding bounds for the head / 1x1 / dense-small kernel tests (test_head_gpu.py, test_conv1x1_gpu.py,
# test_kernel_bounds_cpu.py): inputs, float64 references and per-element worst-case bounds, shared by the GPU tests and
# by the CPU proof that a correct float32 evaluation passes them and a wrong one does not
# ---------------------------------------------------------------------------------------------------------------------------
U32 = 2.0 ** -24                    # unit roundoff of float32: one correctly rounded operation errs by at most U32 * |result|
COSINE_EPS = float(np.float32(1e-12))          # the clamp as the kernel receives it (a C float)


def rounding_bound(*parts):
    """``2^-24 * sum_i c_i * A_i``: ``A_i`` the float64 sum of the absolute values of a group of terms an element adds up, ``c_i`` the
    length of the longest chain of float32 roundings between those terms and the stored element."""
    return U32 * sum(float(c) * A for c, A in parts)


def bound_ratio(got, ref, bound):
    """|got - ref| / bound per element; where the bound is 0 (every term is 0) only an exact result passes; NaN counts as inf."""
    err = (got.double() - ref).abs()
    exact0 = torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float('inf')))
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), exact0)
    return torch.nan_to_num(ratio, nan=float('inf'), posinf=float('inf'))


def assert_within(got, ref, bound, what):
    """Prints the largest error / bound (the margin a run leaves) and asserts that no element exceeds its bound."""
    ratio = bound_ratio(got.detach().cpu(), ref, bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("error/bound %-34s max %.4f" % (what, worst))
    assert worst <= 1.0, "%s: %d of %d elements beyond their rounding bound, worst error / bound = %g" % (
        what, int((ratio > 1.0).sum()), ratio.numel(), worst)
    return worst


# ---- cosine classifier ------------------------------------------------------------------------------------------------------
# (N, Ch, H, W, K, forward kernel, backward kernel, feat at an element offset of 1): every K on every kernel at least once
HEAD_CASES = [
    (2, 40, 36, 40, 19, 'fwd4<8>', 'bwd4', False), (2, 40, 36, 40, 20, 'fwd4<8>', 'bwd4', False), (2, 40, 36, 40, 21, 'fwd4<8>', 'bwd4', False),
    (2, 36, 36, 40, 19, 'fwd4<4>', 'bwd4', False), (2, 36, 36, 40, 20, 'fwd4<4>', 'bwd4', False), (2, 36, 36, 40, 21, 'fwd4<4>', 'bwd4', False),
    (2, 34, 36, 40, 21, 'fwd', 'bwd4', False), (2, 35, 36, 40, 19, 'fwd', 'bwd4', False),
    (1, 33, 9, 31, 20, 'fwd', 'bwd', False), (1, 33, 9, 31, 19, 'fwd', 'bwd', False),
    (1, 1, 2, 2, 21, 'fwd', 'bwd4', False),
    (1, 40, 36, 40, 21, 'fwd', 'bwd', True), (1, 40, 36, 40, 20, 'fwd', 'bwd', True),
]


def head_paths(Ch, HW, aligned):
    """The launchers' predicates (csrc/head.hip launch_fwd / launch_bwd) restated: which kernels a shape and alignment select."""
    fwd = ('fwd4<8>' if Ch % 8 == 0 else 'fwd4<4>') if (HW % 4 == 0 and Ch % 4 == 0 and aligned) else 'fwd'
    return fwd, ('bwd4' if (HW % 4 == 0 and aligned) else 'bwd')


def head_inputs(N, Ch, H, W, K):
    """(feat [N,Ch,H,W], phat [K,Ch] unit rows in float32, g [N,K,H,W]) with the planted pixels: a zero vector on the first pixel of
    the first image and on the last pixel of the last one, |f| ~ 1e-20 (squares are denormal: the eps clamp) on pixel 1, and on pixel 2
    a multiple of proxy 0 (cosine 1: a logit whose terms all have one sign); the gradient of the first pixel has the signs of the
    proxies' channel 0, so that one feature gradient is a sum of terms of one sign as well."""
    gen = torch.Generator().manual_seed(100000 * N + 1000 * Ch + 10 * K + H)
    f = torch.randn((N, Ch, H, W), generator=gen)
    phat = torch.nn.functional.normalize(torch.randn((K, Ch), generator=gen), dim=1)
    g = torch.randn((N, K, H, W), generator=gen)
    ff = f.view(N, Ch, H * W)
    ff[0, :, 0] = 0.0
    ff[N - 1, :, H * W - 1] = 0.0
    ff[0, :, 1] = torch.randn(Ch, generator=gen).sign() * (1e-20 / Ch ** 0.5)
    ff[0, :, 2] = 3.0 * phat[0]
    gg = g.view(N, K, H * W)
    gg[0, :, 0] = gg[0, :, 0].abs() * torch.where(phat[:, 0] < 0, -1.0, 1.0)       # d/df_0 on the first pixel: terms of one sign too
    return f, phat, g


def head_reference(f, phat, g):
    """float64 evaluation of the kernels' formulas on float32 inputs, with the bounds.

    logit_k = sum_c f_c p_kc / n,  n = max(|f|, eps);  dfeat_c = (sum_k g_k p_kc - (sum_k g_k logit_k) f_c / n) / n.

    Chains of float32 roundings (k_cosine_fwd / k_cosine_bwd and their 4-pixel forms, same operations in the same order):
      logit:  Ch fma steps (the dot product; |f|^2 is a parallel chain of the same length), sqrt, 1/n, the product  -> c = Ch + 3
              over A = sum_c |f_c p_kc| / n.  (Adding the two parallel chains instead of taking the longer one would give 1.5 Ch + 3.)
      dfeat:  two groups of terms.  A1 = sum_k |g_k p_kc| / n: K fma steps, the subtraction and the product by 1/n, or Ch + 3 through
              1/n itself, whichever is longer -> c1 = max(K + 2, Ch + 3).  A2 = sum_k |g_k| (sum_c' |f_c' p_kc'| / n) |f_c| / n^2 (the
              second sum expanded to the products the kernel adds, because the float32 logits carry their own error):
              Ch + 3 roundings in the logit, K fma steps, s / n, times f_c, the subtraction, the product -> c2 = Ch + K + 7.
    Returns a dict of float64 tensors shaped like the kernel's outputs."""
    N, Ch, H, W = f.shape
    K = phat.shape[0]
    fd, pd, gd = f.double().reshape(N, Ch, H * W), phat.double(), g.double().reshape(N, K, H * W)
    n = fd.pow(2).sum(1).sqrt().clamp_min(COSINE_EPS)[:, None]                     # [N,1,HW]
    logits = torch.einsum('nch,kc->nkh', fd, pd) / n
    A_logit = torch.einsum('nch,kc->nkh', fd.abs(), pd.abs()) / n
    s = (gd * logits).sum(1, keepdim=True)
    df = (torch.einsum('nkh,kc->nch', gd, pd) - s * fd / n) / n
    A1 = torch.einsum('nkh,kc->nch', gd.abs(), pd.abs()) / n
    A2 = (gd.abs() * A_logit).sum(1, keepdim=True) * fd.abs() / (n * n)
    return {'n': n.reshape(N, H, W), 'zero': (fd.abs().sum(1) == 0).reshape(N, H, W),
            'logits': logits.reshape(N, K, H, W), 'logits_bound': rounding_bound((Ch + 3, A_logit)).reshape(N, K, H, W),
            'dfeat': df.reshape(N, Ch, H, W), 'dfeat_bound': rounding_bound((max(K + 2, Ch + 3), A1), (Ch + K + 7, A2)).reshape(N, Ch, H, W),
            # a zero feature vector as the kernel documents it: n = eps, dfeat_c = (sum_k g_k p_kc) / eps; K fma steps, 1/eps, the
            # subtraction of an exact 0 and the product -> c = K + 3
            'dfeat_zero': (torch.einsum('nkh,kc->nch', gd, pd) / COSINE_EPS).reshape(N, Ch, H, W),
            'dfeat_zero_bound': rounding_bound((K + 3, torch.einsum('nkh,kc->nch', gd.abs(), pd.abs()) / COSINE_EPS)).reshape(N, Ch, H, W)}


# ---- dense small: y = x w^T, dx = dy w, dw = dy^T x ---------------------------------------------------------------------------
DENSE_CASES = [(4, 2048, 256), (3, 70, 13), (1, 1, 1), (5, 300, 7)]


def dense_inputs(N, K, M):
    """x [N,K], w [M,K], dy [N,M]; row 0 of x carries the signs of row 0 of w: y[0,0] is a sum of terms of one sign."""
    gen = torch.Generator().manual_seed(10000 * N + 10 * K + M)
    x, w, dy = torch.randn((N, K), generator=gen), torch.randn((M, K), generator=gen) / K ** 0.5, torch.randn((N, M), generator=gen)
    x[0] = x[0].abs() * torch.where(w[0] < 0, -1.0, 1.0)
    return x, w, dy


def dense_reference(x, w, dy):
    """float64 products and bounds.  k_dense_fwd: a lane adds every 64th product with fma (ceil(K / 64) roundings), then six butterfly
    additions -> c = ceil(K / 64) + 6 over A = sum_k |x_k w_k|.  k_dense_bwd_x: M fma steps in order -> c = M over sum_m |dy_m w_mk|.
    k_dense_bwd_w: N fma steps -> c = N over sum_n |dy_nm x_nk|."""
    (N, K), M = x.shape, w.shape[0]
    xd, wd, gd = x.double(), w.double(), dy.double()
    return {'y': xd @ wd.t(), 'y_bound': rounding_bound(((K + 63) // 64 + 6, xd.abs() @ wd.abs().t())),
            'dx': gd @ wd, 'dx_bound': rounding_bound((M, gd.abs() @ wd.abs())),
            'dw': gd.t() @ xd, 'dw_bound': rounding_bound((N, gd.abs().t() @ xd.abs()))}


# ---- 1x1 convolution with the folded BatchNorm / residual / ReLU epilogue -----------------------------------------------------------
# (N, K, M, H, W, residual, relu, epilogue)
CONV1X1_CASES = [(2, 8, 64, 36, 40, True, False, True), (1, 8, 32, 4, 2305, False, True, True), (1, 4, 64, 4, 2048, True, True, True),
                 (2, 12, 32, 1, 4, False, False, True), (1, 8, 64, 36, 40, False, False, False)]


def conv1x1_tiles(M, HW):
    """(ptiles, mtiles) of mas_conv1x1_fwd: pixel tiles of 256 lanes x 4 pixels, output-channel tiles of 32."""
    return (HW + 1023) // 1024, M // 32


def conv1x1_inputs(N, K, M, H, W, res):
    """x, the [M,K] weight, BatchNorm (weight, bias, running_mean, running_var), residual or None."""
    gen = torch.Generator().manual_seed(1000 * K + 10 * M + N + H)
    x = torch.randn((N, K, H, W), generator=gen)
    w = torch.randn((M, K), generator=gen)
    bn = (torch.rand(M, generator=gen) + 0.5, torch.randn(M, generator=gen), torch.randn(M, generator=gen), torch.rand(M, generator=gen) + 0.3)
    return x, w, bn, (torch.randn((N, M, H, W), generator=gen) if res else None)


def conv1x1_reference(x, w, scale, shift, res, relu):
    """float64 relu?(scale * sum_k x_k w_mk + shift + res) on float32 inputs (scale / shift None: the bare sum) and its bound:
    K fma steps, the product by scale, the addition of shift, the addition of the residual -> c = K + 3 (K for the bare form) over
    A = |scale| sum_k |x_k w_mk| + |shift| + |res|.  ReLU rounds nothing and cannot grow an error."""
    N, K, H, W = x.shape
    xd, wd = x.double().reshape(N, K, H * W), w.double()
    y, A, c = torch.einsum('nkh,mk->nmh', xd, wd), torch.einsum('nkh,mk->nmh', xd.abs(), wd.abs()), K
    if scale is not None:
        s, t = scale.double()[None, :, None], shift.double()[None, :, None]
        y, A, c = y * s + t, A * s.abs() + t.abs(), K + 3
        if res is not None:
            y, A = y + res.double().reshape(N, -1, H * W), A + res.double().abs().reshape(N, -1, H * W)
        if relu:
            y = y.clamp_min(0.0)
    return y.reshape(N, -1, H, W), rounding_bound((c, A)).reshape(N, -1, H, W)


# ---------------------------------------------------------------------------------------------------------------------------
# BatchNorm + ReLU + residual (csrc/bn.hip): the launcher's group / chunk arithmetic restated, inputs, and float64 references
# with per-element bounds, split in two so that every bound follows from the kernels' order of operations:
#   (a) the statistics against float64 of the float32 input (bn_stats_reference),
#   (b) the apply and backward kernels against float64 evaluations of their formulas with the float32 inputs and the DEVICE's
#       float32 statistics taken as given (bn_apply_reference, bn_backward_reference).
# test_bn_gpu.py uses them on the device's results, test_kernel_bounds_cpu.py on a float32 restatement in the kernels' order.
# ---------------------------------------------------------------------------------------------------------------------------
UD = 2.0 ** -53                     # unit roundoff of double
BN_THREADS = 256
BN_GROUPS_PER_CHUNK = 2048          # kChunk = 8192 elements of a plane per workgroup of the reduction kernels
BN_UNROLL = 4                       # groups k_bn_bwd_partial keeps in flight per thread

# (N, C, H, W) -> what the case is in the table for (bn_paths of the shape on a 16-byte aligned tensor must say exactly this).
# chunks: reduction workgroups per plane; a: the misalignments its planes take; second: what chunk 1 holds, per misalignment
# ('empty', 'boundary': one group that the plane covers in part, 'full': one group inside the plane); no_full: no plane has a whole
# group; dup: some thread of k_bn_bwd_partial takes the clamped duplicate; two_trips: some thread runs its four-group loop twice.
BN_CASES = [
    ((2, 5, 1, 8193), dict(chunks=2, a={0, 1, 2, 3}, second={0: 'boundary', 1: 'boundary', 2: 'boundary', 3: 'full'}, no_full=False, dup=True, two_trips=True)),
    ((2, 5, 1, 8191), dict(chunks=2, a={0, 1, 2, 3}, second={0: 'empty', 1: 'empty', 2: 'boundary', 3: 'boundary'}, no_full=False, dup=True, two_trips=True)),
    ((2, 3, 64, 128), dict(chunks=2, a={0}, second={0: 'empty'}, no_full=False, dup=False, two_trips=True)),
    ((1, 2, 1, 4100), dict(chunks=1, a={0}, second={}, no_full=False, dup=True, two_trips=True)),
    ((1, 5, 33, 37), dict(chunks=1, a={0, 1, 2, 3}, second={}, no_full=False, dup=True, two_trips=False)),
    ((3, 5, 1, 3), dict(chunks=1, a={0, 1, 2, 3}, second={}, no_full=True, dup=False, two_trips=False)),
    ((2, 4, 1, 2), dict(chunks=1, a={0, 2}, second={}, no_full=True, dup=False, two_trips=False)),
    ((4, 6, 1, 1), dict(chunks=1, a={0, 1, 2, 3}, second={}, no_full=True, dup=False, two_trips=False)),
]
BN_OPTION_CASES = [BN_CASES[0][0], BN_CASES[4][0], BN_CASES[5][0]]       # the cases every option runs on
# one option at a time on top of relu + residual
BN_OPTIONS = ['affine_false', 'no_running_stats', 'residual_no_grad', 'frozen_weight', 'frozen_bias', 'no_relu', 'momentum_0.01',
              'momentum_1.0', 'eps_1e-3', 'two_steps']


def bn_max_groups(HW):
    return (HW + 3) // 4 + 1


def bn_chunks(HW):
    return (bn_max_groups(HW) + BN_GROUPS_PER_CHUNK - 1) // BN_GROUPS_PER_CHUNK


def bn_plane_groups(a, HW, chunks):
    """groups_of and the chunk loop of k_bn_partial / k_bn_bwd_partial for one plane at misalignment a: per chunk
    (lo, hi, flo, fhi): groups [lo, hi) of the plane fall into the chunk, [flo, fhi) of them lie whole inside the plane."""
    n = (a + HW + 3) >> 2
    first_full, end_full = (a + 3) >> 2, (a + HW) >> 2
    out = []
    for k in range(chunks):
        lo = k * BN_GROUPS_PER_CHUNK
        hi = max(lo, min(n, lo + BN_GROUPS_PER_CHUNK))
        flo, fhi = max(lo, first_full), min(hi, end_full)
        out.append((lo, hi, flo, max(flo, fhi)))
    return n, out


def bn_paths(N, C, HW, offset=0):
    """The predicates of BN_CASES for a contiguous [N,C,HW] tensor whose first element lies `offset` elements past a 16-byte boundary."""
    chunks = bn_chunks(HW)
    got = dict(chunks=chunks, a=set(), second={}, no_full=True, dup=False, two_trips=False, per_thread=0)
    for p in range(N * C):
        a = (offset + p * HW) & 3
        got['a'].add(a)
        n, per_chunk = bn_plane_groups(a, HW, chunks)
        assert n <= bn_max_groups(HW)                                           # (the grid and the mask row cover every group)
        for k, (lo, hi, flo, fhi) in enumerate(per_chunk):
            full = fhi - flo
            got['no_full'] &= full == 0
            got['dup'] |= full % (BN_UNROLL * BN_THREADS) != 0
            got['two_trips'] |= full > BN_UNROLL * BN_THREADS
            got['per_thread'] = max(got['per_thread'], (hi - lo + BN_THREADS - 1) // BN_THREADS)
            if k == 1:
                what = 'empty' if hi == lo else ('full' if full == 1 else 'boundary')
                assert hi - lo <= 1 and got['second'].get(a, what) == what
                got['second'][a] = what
    return got


def bn_inputs(N, C, H, W, seed=0, const=None):
    """x (mean 0.5, std 2; or the constant `const`), residual, upstream gradient, gamma, beta, running mean, running variance."""
    gen = torch.Generator().manual_seed(100003 * N + 1009 * C + 31 * H + W + 7919 * seed)
    shape = (N, C, H, W)
    x = torch.randn(shape, generator=gen) * 2 + 0.5 if const is None else torch.full(shape, float(const))
    return dict(x=x, res=torch.randn(shape, generator=gen), dy=torch.randn(shape, generator=gen), gamma=torch.rand(C, generator=gen) + 0.5,
                beta=torch.randn(C, generator=gen) * 0.3, rm=torch.randn(C, generator=gen) * 0.1, rv=torch.rand(C, generator=gen) + 0.5)


def bn_conditioning_input():
    """[2,4,1,1221]: unit-variance channels with mean / std of 0, 1, 8 and 64."""
    gen = torch.Generator().manual_seed(1221)
    return torch.randn((2, 4, 1, 1221), generator=gen) + torch.tensor([0.0, 1.0, 8.0, 64.0]).view(1, 4, 1, 1)


def f32_as_float(v):
    """The double a C float parameter holds."""
    return float(np.float32(v))


def bn_stats_reference(x, eps, momentum=None, rm0=None, rv0=None, c_s=10, c_q=11, c_d=None):
    """(a) mean, invstd and the updated running statistics of k_bn_partial + k_bn_stats in float64, with bounds.

    The kernel: S = sum x, Q = sum x^2 per channel, m = S / n, var = max(Q / n - m^2, 0), invstd = 1 / sqrt(var + eps), all in double
    from the per-thread float32 sums on.  A thread of k_bn_partial adds at most 8 groups per chunk (2048 groups, 256 threads), each
    pre-summed in two levels, (x0 + x1) + (x2 + x3): 2 + 8 roundings on any element's way into S, c_s = 10 over mean|x|; one more for
    the square on the way into Q, c_q = 11 over mean(x^2).  The double part (six shuffle steps, three adds over the waves, the
    partials in index order: c_d = per_channel + 9 roundings of 2^-53) is carried as well.
      mean:    dS + u |m|                                   (the cast)
      var:     dvar = dQ + 2 |m| dS + dS^2                   (+ four double roundings of Q / n - m^2)
      invstd:  the device's variance lies in [max(var - dvar, 0), var + dvar] and 1 / sqrt(. + eps) falls monotonically, so the error is at
               most 1 / sqrt(max(var - dvar, 0) + eps) - invstd -- the factor dvar / (2 (var + eps)) with its whole remainder -- plus
               the cast of a value no larger than that.
      running: (1 - mom) r + mom m and (1 - mom) r + mom var n / (n - 1) in double: mom dS, mom n / (n - 1) dvar, plus the cast.
    The bound on invstd is what the one-pass form can lose: dvar / var grows with (mean / std)^2 (test_bn_gpu.py: conditioning).
    Other callers: c_s = c_q = 0 for partials that are exact (k_bn_stats_wide), c_d the double chain of that kernel."""
    N, C = x.shape[:2]
    xd = x.double().transpose(0, 1).reshape(C, -1)
    n = xd.shape[1]
    if c_d is None:
        c_d = N * bn_chunks(n // N) + 9
    m, A1, q = xd.mean(1), xd.abs().mean(1), (xd * xd).mean(1)
    var = (xd - m[:, None]).pow(2).mean(1)
    dS = (c_s * U32 + c_d * UD) * A1
    dQ = (c_q * U32 + c_d * UD) * q
    dvar = dQ + 2 * m.abs() * dS + dS * dS + 4 * UD * (q + m * m)
    e = f32_as_float(eps)
    invstd = (var + e).rsqrt()
    worst = ((var - dvar).clamp_min(0.0) + e).rsqrt()
    out = dict(mean=m, mean_bound=dS + U32 * m.abs(), var=var, dvar=dvar, invstd=invstd, invstd_bound=(worst - invstd) + (U32 + 3 * UD) * worst)
    if momentum is not None:
        mom = f32_as_float(momentum)
        unb = n / (n - 1.0) if n > 1 else 1.0
        rm = (1.0 - mom) * rm0.double() + mom * m
        rv = (1.0 - mom) * rv0.double() + mom * var * unb
        out.update(rm=rm, rm_bound=mom * dS + U32 * rm.abs() + 4 * UD * (rm0.double().abs() + m.abs()),
                   rv=rv, rv_bound=mom * unb * dvar + U32 * rv.abs() + 4 * UD * (rv0.double().abs() + var * unb))
    return out


def _per_channel(t, C, default):
    return torch.full((1, C, 1, 1), default, dtype=torch.float64) if t is None else t.detach().double().cpu().view(1, C, 1, 1)


def bn_apply_reference(x, gamma, beta, res, stat1, stat2, relu, eps=None):
    """(b) k_bn_apply: y = relu?(((x - mu) * is) * gamma + beta + res) in float64 on float32 operands.  Training (eps None): stat1 / stat2
    are the device's float32 mean / invstd.  Five roundings (the subtraction, two products, two additions) over
    A = |xhat gamma| + |beta| + |res|.  Inference: stat2 is the running variance, is = 1 / sqrtf(var + eps): three more roundings (the
    addition, the square root, the division) on the first term.  ReLU rounds nothing and cannot grow an error.  -> (y, bound)"""
    C = x.shape[1]
    mu, gm, b = _per_channel(stat1, C, 0.0), _per_channel(gamma, C, 1.0), _per_channel(beta, C, 0.0)
    if eps is None:
        inv, extra = _per_channel(stat2, C, 0.0), 0
    else:
        inv, extra = (_per_channel(stat2, C, 0.0) + f32_as_float(eps)).rsqrt(), 3
    t = (x.double() - mu) * inv * gm
    r = torch.zeros_like(t) if res is None else res.double()
    y = t + b + r
    bound = U32 * (5 * (t.abs() + b.abs() + r.abs()) + extra * t.abs())
    return (y.clamp_min(0.0) if relu else y), bound


def bn_backward_reference(x, dy, y_dev, gamma, mean, invstd, relu, per_thread=8, per_channel=None):
    """(b) k_bn_bwd_partial + k_bn_bwd_stats + k_bn_bwd_apply in float64 on float32 operands, the device's float32 mean / invstd / y:
      g = dy [y > 0] (exact),  xhat = (x - mu) is,  dbeta = sum g,  dgamma = sum g xhat,
      dx = k (g - mean g - xhat mean(g xhat)),  k = gamma is,  dres = g.
    A thread adds the four elements of at most `per_thread` = 8 groups one after the other in float32: 32 additions; g xhat takes three
    roundings first; the rest is double (c_d roundings of 2^-53) and one cast:  dbeta: 33 over sum|g|,  dgamma: 36 over sum|g xhat|.
    dx: the two subtractions, the product by k and k's own rounding on every term, the subtraction and two products of xhat mean(g xhat)
    on the last: 6 over |k| (|g| + |mean g| + |xhat mean(g xhat)|); the float32 coefficients mean g and mean(g xhat) carry the errors of
    the sums divided by the count (their cast is the one counted in the sums' bounds): |k| (d_mg + |xhat| d_mgx) more.
    -> dict(dres, dbeta, dbeta_bound, dgamma, dgamma_bound, dx, dx_bound)"""
    N, C, H, W = x.shape
    n = N * H * W
    if per_channel is None:
        per_channel = N * bn_chunks(H * W)
    c_d = per_channel + 9
    mu, inv, gm = _per_channel(mean, C, 0.0), _per_channel(invstd, C, 0.0), _per_channel(gamma, C, 1.0)
    g32 = torch.where(y_dev.detach().cpu() > 0, dy, torch.zeros_like(dy)) if relu else dy
    g = g32.double()
    xhat = (x.double() - mu) * inv
    red = lambda t: t.sum((0, 2, 3))
    dbeta, dgamma = red(g), red(g * xhat)
    dbeta_bound = ((4 * per_thread + 1) * U32 + c_d * UD) * red(g.abs())
    dgamma_bound = ((4 * per_thread + 4) * U32 + c_d * UD) * red((g * xhat).abs())
    v = lambda t: t.view(1, C, 1, 1)
    mg, mgx, k = v(dbeta) / n, v(dgamma) / n, gm * inv
    dx = k * (g - mg - xhat * mgx)
    dx_bound = k.abs() * (6 * U32 * (g.abs() + mg.abs() + (xhat * mgx).abs()) + v(dbeta_bound) / n + xhat.abs() * v(dgamma_bound) / n)
    return dict(dres=g32, dbeta=dbeta, dbeta_bound=dbeta_bound, dgamma=dgamma, dgamma_bound=dgamma_bound, dx=dx, dx_bound=dx_bound)


# ---------------------------------------------------------------------------------------------------------------------------
# bilinear upsampling (csrc/upsample.hip): make_tap restated in torch float32 operation by operation (nothing is contracted: the
# same bits as the kernel's), the weights built from those taps, combined in float64
# ---------------------------------------------------------------------------------------------------------------------------
UPSAMPLE_MAX_TAPS = 16
# (N, C, Hi, Wi, Ho, Wo) -> the kernel forms the case selects on 16-byte aligned tensors (upsample_paths must say exactly this).
# fast4: k_upsample_bwd<true>; fast_cols: input columns that take its three-load form (the interior ones: 0 and Wi - 1 stay on the
# tested loop); fwd_cols / bwd_cols: block columns of the forward (1024 outputs) and of the backward (64 inputs);
# bwd_partial: the last backward block column is partial; vec_store: the forward stores float4; cols: the largest number of candidate
# output columns of an input column (the tap limit Wo = 6 Wi fills all 16, the fractional 17 / 3 reaches 15; None: not what the case
# is for); single: every tap has i1 == i0 (one input pixel)
UPSAMPLE_CASES = [
    ((1, 2, 2, 260, 8, 1040), dict(fast4=True, fast_cols=258, fwd_cols=2, bwd_cols=5, bwd_partial=True, vec_store=True, cols=12, single=False)),
    ((1, 2, 3, 5, 12, 20), dict(fast4=True, fast_cols=3, fwd_cols=1, bwd_cols=1, bwd_partial=True, vec_store=True, cols=12, single=False)),
    ((1, 1, 5, 13, 17, 49), dict(fast4=False, fast_cols=0, fwd_cols=1, bwd_cols=1, bwd_partial=True, vec_store=False, cols=None, single=False)),
    ((1, 2, 4, 3, 4, 18), dict(fast4=False, fast_cols=0, fwd_cols=1, bwd_cols=1, bwd_partial=True, vec_store=False, cols=16, single=False)),
    ((1, 2, 4, 3, 5, 17), dict(fast4=False, fast_cols=0, fwd_cols=1, bwd_cols=1, bwd_partial=True, vec_store=False, cols=15, single=False)),
    ((1, 1, 1, 1, 3, 5), dict(fast4=False, fast_cols=0, fwd_cols=1, bwd_cols=1, bwd_partial=True, vec_store=False, cols=None, single=True)),
    ((2, 3, 7, 5, 7, 5), dict(fast4=False, fast_cols=0, fwd_cols=1, bwd_cols=1, bwd_partial=True, vec_store=False, cols=None, single=False)),
]


def upsample_taps(n_in, n_out):
    """make_tap(scale, o, n_in) for o = 0 .. n_out - 1 -> (i0, i1 int64, l0, l1 float32), scale = (float)n_in / (float)n_out."""
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    s = scale * (torch.arange(n_out, dtype=torch.float32) + 0.5) - 0.5
    s = torch.where(s < 0, torch.zeros_like(s), s)
    i0 = s.to(torch.int64)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    l1 = s - i0.to(torch.float32)
    return i0, i1, 1.0 - l1, l1


def upsample_weights(n_in, n_out, dtype):
    """[n_out, n_in]: row o holds l0 at i0 and l1 at i1, added where the two coincide -- in float64 (the forward adds the two products) or
    in float32 (the backward adds the two weights in float32 before it uses them)."""
    i0, i1, l0, l1 = upsample_taps(n_in, n_out)
    w = torch.zeros((n_out, n_in), dtype=dtype)
    o = torch.arange(n_out)
    w[o, i0] += l0.to(dtype)
    w[o, i1] += l1.to(dtype)
    return w


def upsample_out_range(n_in, n_out):
    """out_range of k_upsample_bwd for every input index, in float32 as the kernel -> (lo, hi) int64 [n_in]."""
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    inv = 1.0 / scale
    i = torch.arange(n_in, dtype=torch.float32)
    lo = torch.floor((i - 0.5) * inv - 0.5).to(torch.int64) - 1
    hi = torch.ceil((i + 1.5) * inv - 0.5).to(torch.int64) + 1
    return lo.clamp_min(0), hi.clamp_max(n_out - 1)


def upsample_paths(Hi, Wi, Ho, Wo, gy_aligned=True):
    """The launchers' and kernels' predicates restated.  Also asserts what the backward needs to be right at all: every output column
    that carries weight for an input column is among its (at most 16) candidates, and every such row is in its row range."""
    wx, wy = upsample_weights(Wi, Wo, torch.float32), upsample_weights(Hi, Ho, torch.float32)
    xlo, xhi = upsample_out_range(Wi, Wo)
    ylo, yhi = upsample_out_range(Hi, Ho)
    ox, oy = torch.arange(Wo)[:, None], torch.arange(Ho)[:, None]
    assert bool(((wx == 0) | ((ox >= xlo[None]) & (ox <= torch.minimum(xhi, xlo + UPSAMPLE_MAX_TAPS - 1)[None]))).all())
    assert bool(((wy == 0) | ((oy >= ylo[None]) & (oy <= yhi[None]))).all())
    i0, i1, _, _ = upsample_taps(Wi, Wo)
    j0, j1, _, _ = upsample_taps(Hi, Ho)
    cols = (torch.minimum(xhi, xlo + UPSAMPLE_MAX_TAPS - 1) - xlo + 1)
    fast4 = Wo == 4 * Wi and gy_aligned
    ix = torch.arange(Wi)
    fast = (ix >= 1) & (ix + 2 <= Wi) & (xlo == 4 * ix - 4)
    if fast4:       # what the three loads stand for: exactly the candidates 2 .. 9 carry weight
        k = torch.arange(UPSAMPLE_MAX_TAPS)[:, None]
        w = torch.where(xlo[None] + k <= xhi[None], wx[(xlo[None] + k).clamp_max(Wo - 1), ix[None]], torch.zeros(()))
        assert bool((((w != 0) == ((k >= 2) & (k <= 9))) | ~fast[None]).all())
    return dict(fast4=fast4, fast_cols=int(fast.sum()) if fast4 else 0, fwd_cols=(Wo + 1023) // 1024, bwd_cols=(Wi + 63) // 64, bwd_partial=Wi % 64 != 0,
                vec_store=Wo % 4 == 0, cols=int(cols.max()), single=bool((i0 == i1).all() and (j0 == j1).all()),
                col_count=cols, row_count=(wy != 0).sum(0))


def upsample_reference(x, Ho, Wo):
    """y = Wy x Wx^T in float64 from the float32 taps; k_upsample_fwd computes l0h (l0w v00 + l1w v01) + l1h (l0w v10 + l1w v11) with
    every operation rounded: a product, the inner addition, the product by the row weight, the outer addition -> c = 4 over
    A = sum w |v|."""
    Hi, Wi = x.shape[2:]
    wy, wx = upsample_weights(Hi, Ho, torch.float64), upsample_weights(Wi, Wo, torch.float64)
    f = lambda t: torch.einsum('oh,nchw,pw->ncop', wy, t, wx)
    return f(x.double()), rounding_bound((4, f(x.double().abs())))


def upsample_backward_reference(g, Hi, Wi):
    """gx = Wy^T g Wx in float64 from the float32 weights of k_upsample_bwd (the forward's, transposed; where a tap's two indices
    coincide the kernel adds l0 + l1 in float32, as upsample_weights does).  An input pixel adds, with fma, one term per candidate column
    into a row sum (zero weights skipped or, on the x4 form, absent) and one row sum per contributing row: c = candidate columns +
    contributing rows over A = sum w |g|."""
    Ho, Wo = g.shape[2:]
    wy, wx = upsample_weights(Hi, Ho, torch.float32).double(), upsample_weights(Wi, Wo, torch.float32).double()
    p = upsample_paths(Hi, Wi, Ho, Wo)
    c = (p['row_count'][:, None] + p['col_count'][None, :]).double()
    f = lambda t: torch.einsum('oh,ncop,pw->nchw', wy, t, wx)
    return f(g.double()), U32 * c[None, None] * f(g.double().abs())


def upsample_inputs(N, C, Hi, Wi, Ho, Wo):
    gen = torch.Generator().manual_seed(100003 * Hi + 1009 * Wi + 31 * Ho + Wo)
    return torch.randn((N, C, Hi, Wi), generator=gen), torch.randn((N, C, Ho, Wo), generator=gen)

"""Images past 480x640, model level: the DETR encoder attends over ceil(H / 32) ceil(W / 32) tokens, and every length past 320
(a 640x640 batch: 400, one 800x1088 image: 850) failed inside the transformer with hipError 1 until the streaming attention
kernels (attention.hip attn_long_kernel / attn_kvl_kernel) took them.  Full configuration against the CPU oracle on the same
weights, with test_full_size_forward_loss_and_matching_vs_oracle's tolerances: precise 1e-3 (Hungarian indices exact), bf16 5e-2
on outputs / 3e-2 on the loss."""
import os

import numpy as np
import pytest
import torch

from tests import synth
from tests.test_model_cpu import build_small, nested
from tests.test_model_gpu import full_model, rel, _faithful_oracle, _cmp_grads, GRAD_SAMPLE

pytestmark = pytest.mark.gpu
DEV = 'cuda'
VF = 10000
KEYS = ('pred_boxes', 'pred_relevance_logits', 'detr_hs', 'answer_logits')


@pytest.fixture()
def rt():
    import gpv1_amd.ops as ops
    import gpv1_amd.hip as hip
    hip.lib()
    yield ops.RT
    ops.RT.set_precise(False)


def _images(sizes, seed=3):
    """HxWx3 float images of the given sizes, padded to the batch maximum as inference.predict pads them"""
    from gpv1_amd.misc import nested_tensor_from_tensor_list
    g = torch.Generator().manual_seed(seed)
    raw = [torch.randn(3, h, w, generator=g) for h, w in sizes]
    nt = nested_tensor_from_tensor_list([r.to(DEV) for r in raw])
    return raw, nt.tensors, nt.mask


def _targets(Bf):
    tg = [{'task': 'CocoCaptioning', 'answer': ' '.join(f'w{(37 * j) % (VF - 4)}' for j in range(18))},
          {'task': 'CocoDetection', 'boxes': torch.tensor([[0.5, 0.5, 0.2, 0.3], [0.3, 0.6, 0.1, 0.15], [0.7, 0.3, 0.25, 0.2]], device=DEV),
           'labels': torch.zeros(3, dtype=torch.long, device=DEV)}]
    return tg[:Bf]


def _oracle_cfg():
    cfg = synth.model_cfg(vocab=synth.make_vocab(VF))
    cfg['detr']['dropout'] = 0.0
    cfg['_cls_id'] = VF - 3
    return cfg


def _forward_vs_oracle(rt, sizes):
    import gpv1_amd.hip as hip
    from oracle import gpv_oracle as O
    Bf = len(sizes)
    model = full_model(VF, dropout=0.0)
    model.bert.model.p = 0.0
    model.train()
    _, images, mask = _images(sizes)
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(1000, 30000, (Bf, 6), generator=g).to(DEV)
    attn = torch.ones(Bf, 6, dtype=torch.long, device=DEV)
    tg = _targets(Bf)
    _, tok = model.encode_answers(tg)
    for i, t in enumerate(tg):
        t['answer_token_ids'] = tok[i, 1:]
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    cfg = _oracle_cfg()
    Pm = {k: v.detach().float().cpu().contiguous() for k, v in model.state_dict().items()}
    tg_cpu = [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in t.items()} for t in tg]
    with torch.no_grad():
        ref = O.gpv_forward(Pm, cfg, images.cpu(), mask.cpu(), ids.cpu(), attn.cpu(), tok.cpu(), training=True)
        ref_loss, _ = O.gpv_criterion(ref, tg_cpu, cfg['losses'])
        det = [i for i, t in enumerate(tg_cpu) if t['task'] == 'CocoDetection']
        ref_ind = O.hungarian_match(ref['pred_relevance_logits'][det[0]:det[0] + 1], ref['pred_boxes'][det[0]:det[0] + 1],
                                    tg_cpu[det[0]:det[0] + 1])[0] if det else None
    for precise, otol, ltol in ((True, 1e-3, 1e-3), (False, 5e-2, 3e-2)):
        rt.set_precise(precise)
        with torch.no_grad():
            out = model._forward_impl(nested(images, mask), (ids, attn), tok, None)
            loss = model.criterion(out, tg)[0]
        for k in KEYS:
            e = rel(out[k], ref[k])
            assert e < otol, (precise, k, e)
        assert abs(float(loss) - float(ref_loss)) <= ltol * abs(float(ref_loss)), (precise, float(loss), float(ref_loss))
        if precise and ref_ind is not None:
            ind = model.criterion.localization_criterion.set_criterion.last_indices
            assert len(ind) == 1 and torch.equal(ind[0][0], ref_ind[0][0]) and torch.equal(ind[0][1], ref_ind[0][1]), (ind, ref_ind)
    rt.set_precise(False)
    return model


def test_mixed_orientation_pair_vs_oracle_and_predict(rt):
    """a 480x640 and a 640x480 image pad to 640x640: 400 encoder tokens (the two padding layouts: last 5 rows / last 5 columns)"""
    from gpv1_amd.inference import predict
    model = _forward_vs_oracle(rt, [(480, 640), (640, 480)])
    model.eval()
    imgs = [np.random.RandomState(i).rand(*s, 3).astype(np.float32) * 255 for i, s in enumerate([(480, 640), (640, 480)])]
    g = torch.Generator().manual_seed(12)
    queries = (torch.randint(1000, 30000, (2, 6), generator=g).to(DEV), torch.ones(2, 6, dtype=torch.long, device=DEV))
    for precise in (True, False):
        rt.set_precise(precise)
        with torch.no_grad():
            pred = predict(model, imgs, queries, num_output_boxes=5)
        assert len(pred) == 2
    rt.set_precise(False)


def test_one_800x1088_image_vs_oracle(rt):
    """25 x 34 C5 cells: 850 encoder tokens"""
    _forward_vs_oracle(rt, [(800, 1088)])


def test_precise_training_step_on_a_640x640_pair_vs_fp32_oracle(rt):
    """loss within 1e-3 and weight gradients (cosine >= 0.999, norm within 1 %; 2 % in the backbone) against the fp32 oracle's
    autograd, the attention in-projections of the encoder and the decoder included"""
    rt.set_precise(True)
    model = full_model(VF, dropout=0.0)
    model.bert.model.p = 0.0
    model.train()
    _, images, mask = _images([(480, 640), (640, 480)])
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(1000, 30000, (2, 6), generator=g).to(DEV)
    attn = torch.ones(2, 6, dtype=torch.long, device=DEV)
    tg = _targets(2)
    _, tok = model.encode_answers(tg)
    for i, t in enumerate(tg):
        t['answer_token_ids'] = tok[i, 1:]
    out = model._forward_impl(nested(images, mask), (ids, attn), tok, None)
    loss = model.criterion(out, tg)[0]
    loss.backward()
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    tg_cpu = [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in t.items()} for t in tg]
    names = list(GRAD_SAMPLE) + [n for n, _ in model.named_parameters() if n.endswith('in_proj_weight')
                                 and ('encoder.layers.0.' in n or 'encoder.layers.5.' in n or 'decoder.layers.0.' in n)]
    assert any('encoder' in n for n in names) and any('decoder' in n for n in names), names
    ref, ref_loss, gref = _faithful_oracle(model, _oracle_cfg(), images, mask, ids, attn, tok, tg_cpu, names, faithful=False)
    assert abs(float(loss) - float(ref_loss)) <= 1e-3 * abs(float(ref_loss)), (float(loss), float(ref_loss))
    rep = _cmp_grads(model, gref, {})
    bad = {n: v for n, v in rep.items() if v[2] >= 1e-3 and (v[1] < 0.999 or v[0] > (0.02 if 'backbone' in n else 0.01))}
    assert not bad, bad
    rt.set_precise(False)


def test_graphed_train_step_at_640x640_equals_eager(rt):
    """train.FlatTrainer's graphed body against the eager step on 640x640 batches (400 tokens), as
    test_graphed_train_step_equals_eager does at the small size"""
    from gpv1_amd.train import FlatTrainer
    from tests.test_model_cpu import V, B
    rt.set_precise(False)
    images, mask, ids, attn = synth.synth_batch(B, 640, 640, 5, V, pad_to=[(480, 640), (640, 480), (640, 640), (600, 620)])
    images, mask, ids, attn = images.to(DEV), mask.to(DEV), ids.to(DEV), attn.to(DEV)
    cap = [{'task': 'CocoCaptioning', 'answer': ' '.join(f'w{(3 * i + j) % (V - 4)}' for j in range(4))} for i in range(B)]
    det = [{'task': 'CocoDetection', 'boxes': torch.tensor([[0.5, 0.5, 0.2, 0.3], [0.3, 0.6, 0.1, 0.1]], device=DEV)[: 1 + i % 2],
            'labels': torch.zeros(1 + i % 2, dtype=torch.long, device=DEV)} for i in range(B)]
    mixed = [cap[i] if i % 2 == 0 else det[i] for i in range(B)]
    schedule = [cap, cap, mixed, mixed, det]
    res = {}
    for graphs in (False, True):
        model, _ = build_small()
        model.to(DEV).train()
        model.bert.model.p = 0.0
        tr = FlatTrainer(model, lr=1e-3, lr_backbone=1e-4, graphs=graphs)
        losses = [float(tr.train_step(nested(images, mask), (ids, attn), [dict(t) for t in tg])) for tg in schedule]
        res[graphs] = (losses, tr.P.clone(), len(tr._bodies))
    (l0, p0, n0), (l1, p1, n1) = res[False], res[True]
    assert n0 == 0 and n1 >= 1, (n0, n1)
    assert all(np.isfinite(l0)) and all(np.isfinite(l1))
    for a, b_ in zip(l0, l1):
        assert abs(a - b_) <= 2e-2 * max(abs(a), 1.0), (l0, l1)
    assert rel(p1, p0.cpu()) < 1e-2, rel(p1, p0.cpu())


def test_inference_graph_replay_at_850_tokens_equals_the_eager_call(rt):
    """greedy inference on one 800x1088 image: the captured inference graph (replayed twice) equals the eager call"""
    from tests.test_model_cpu import V
    rt.set_precise(False)
    images, mask, ids, attn = synth.synth_batch(1, 800, 1088, 5, V)
    samples = nested(images.to(DEV), mask.to(DEV))
    q = (ids.to(DEV), attn.to(DEV))
    model, _ = build_small()
    model.to(DEV).eval()
    with torch.no_grad():
        model.cfg['graph_inference'] = False
        eager = model(samples, q, None)
        assert len(model._igraphs) == 0
        model.cfg['graph_inference'] = True
        g1 = model(samples, q, None)
        g2 = model(samples, q, None)
        assert len(model._igraphs) >= 1
    for k in ('pred_boxes', 'pred_relevance_logits', 'answer_logits'):
        assert torch.equal(g1[k], g2[k]), k
        assert torch.isfinite(eager[k].float()).all(), k
        assert rel(g1[k], eager[k].float().cpu()) < 1e-2, (k, rel(g1[k], eager[k].float().cpu()))

"""CPU fp32 restatement of the reference's RetinaNet CLASSIFICATION PRE-TRAINING graph (TEST INFRASTRUCTURE ONLY), built from the pieces of
oracle/retinanet_net_ref.py: RetinaNet.py:81-99 (images - mean), :120-135 (the backbone's last unit -> reduce_mean over H, W -> sparse softmax
cross-entropy, arg-max, accuracy; loss + wd * l2 over the trainables of 'feature_extractor'; Momentum 0.9 WITHOUT the batch-norm update ops).
Layers l0 .. l64 (the first 1 + 4 * sum(block_list) of the detection graph's creation order).  Pinned against the reference's own class run
on oracle/tf_shim: tests/golden/retinanet_pretrain.npz (tests/golden/make_golden_retinanet_pretrain.py)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import retinanet_net_ref as NR
from oracle.ssd300_ref import maxpool_same

BLOCKS = (3, 4, 6, 3)


def num_layers(block_list=BLOCKS):
    return 1 + 4 * sum(block_list)


def specs(block_list=BLOCKS, init_filters=16):
    return NR.layer_specs(block_list, init_filters)[: num_layers(block_list)]


def init_params(seed=0, block_list=BLOCKS):
    """oracle init_params restricted to l0 .. l64 (the backbone's draws come first, so these equal the detection model's l0 .. l64)"""
    nb = num_layers(block_list)
    return {k: v for k, v in NR.init_params(seed, block_list=block_list).items() if int(k[1:].split('.')[0]) < nb}


def forward(p, images_nhwc, training, subtract_mean=True, relu_masks=None, taps=None, block_list=BLOCKS):
    """-> logits [N, 4 * FILTERS[-1]]; batch norms on batch statistics when training, else on the moving statistics (never updated here)"""
    x = images_nhwc.float()
    if subtract_mean:
        x = x - torch.tensor(NR.MEAN_RGB).view(1, 1, 1, 3)
    x = x.permute(0, 3, 1, 2)
    net = NR._Net(p, specs(block_list, p['l0.w'].shape[0]), training, None, relu_masks, taps)
    x = maxpool_same(net.stem(x), 3, 2)
    for blocks in block_list:
        for _ in range(blocks):
            branch = net.conv(net.conv(net.conv(x)))
            x = branch + net.conv(x)
    assert net.i == len(net.specs)
    return x.mean(dim=(2, 3))


def trainable_names(p):
    return NR.trainable_names(p)


def loss_fn(p, images_nhwc, labels, weight_decay=1e-4, relu_masks=None):
    logits = forward(p, images_nhwc, True, relu_masks=relu_masks)
    ce = F.cross_entropy(logits, torch.as_tensor(labels).long().view(-1))
    l2 = sum((p[k] ** 2).sum() / 2 for k in trainable_names(p))
    return ce + weight_decay * l2, ce, logits


def train_step(p, mom, images_nhwc, labels, lr, weight_decay=1e-4, relu_masks=None):
    """one Momentum step in place; -> (total loss, cross-entropy, accuracy, gradients, logits) of the forward pass before the update"""
    names = trainable_names(p)
    for k in names:
        p[k].requires_grad_(True)
        p[k].grad = None
    total, ce, logits = loss_fn(p, images_nhwc, labels, weight_decay, relu_masks)
    total.backward()
    grads = {}
    with torch.no_grad():
        for k in names:
            grads[k] = p[k].grad.clone()
            mom[k].mul_(0.9).add_(p[k].grad)
            p[k].sub_(lr * mom[k])
            p[k].requires_grad_(False)
            p[k].grad = None
    logits = logits.detach()
    pred = logits.argmax(1)                                  # first index of the maximum, as tf.argmax
    acc = float((pred == torch.as_tensor(labels).long().view(-1)).float().mean())
    return float(total.detach()), float(ce.detach()), acc, grads, logits

"""Plain float64 reference of the stride-1 "same" convolutions of csrc/conv.hip (no GPU, no project code): the forward with the kernel's
epilogue in its documented order, the transposed (backward-data) form, and the gradients by autograd.  Tensors are NCHW as torch has
them; the GPU tests permute to the kernels' NHWC.  tests/test_conv_ref_cpu.py pins this file before any kernel is graded against it."""
import torch
import torch.nn.functional as F


def apply_mask(v, m, mask_elu=False):
    """the activation-derivative mask of ConvArgs: v where m > 0, else 0 -- or v * (m + 1) with mask_elu, m being an ELU output"""
    return torch.where(m > 0, v, v * (m + 1) if mask_elu else torch.zeros_like(v))


def conv_forward(x, w, bias=None, relu=0, posmap=None, mask=None, mask_elu=False):
    """x [B,cin,H,W], w [64,cin,ks,ks], bias [64], posmap [64,H,W], mask [B,64,H,W] -> float64 [B,64,H,W]:
    conv + bias, activation (0 none, 1 ReLU, 2 ELU), + posmap, mask"""
    ks = w.shape[-1]
    v = F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), padding=ks // 2)
    return epilogue(v, relu, posmap, mask, mask_elu)


def epilogue(v, relu=0, posmap=None, mask=None, mask_elu=False):
    """everything of conv_forward after conv + bias (so several epilogues can share one float64 convolution)"""
    assert relu in (0, 1, 2)
    if relu == 1:
        v = torch.relu(v)
    elif relu == 2:
        v = F.elu(v)
    if posmap is not None:
        v = v + posmap.double()
    if mask is not None:
        v = apply_mask(v, mask.double(), mask_elu)
    return v


def transposed_weight(w):
    """w [co,ci,ks,ks] -> the weight of the backward-data convolution: taps flipped, ci / co swapped"""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def conv_backward_data(dy, w, mask=None, mask_elu=False):
    """the transposed form as the kernel runs it: a forward convolution of dy with transposed_weight(w), then the mask"""
    return conv_forward(dy, transposed_weight(w), None, 0, None, mask, mask_elu)


def conv_grads(x, w, dy, need_dx=True):
    """autograd in float64 through F.conv2d(x, w, bias, padding=ks//2): (dx or None, dw, db)"""
    ks = w.shape[-1]
    xg = x.double().clone().requires_grad_(need_dx)
    wg = w.double().clone().requires_grad_(True)
    bg = torch.zeros(w.shape[0], dtype=torch.double, requires_grad=True)
    F.conv2d(xg, wg, bg, padding=ks // 2).backward(dy.double())
    return (xg.grad if need_dx else None), wg.grad, bg.grad

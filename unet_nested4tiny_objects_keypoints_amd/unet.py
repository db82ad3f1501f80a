"""Drop-in ``UNet_Nested`` for MI355X: the reference's module API over the HIP path.

Mirrors ``/root/reference/models/unet.py:204-300`` at the ``torch.nn.Module`` boundary -- same
constructor (``UNet_Nested(in_channels=3, n_classes=4, feature_scale=2, is_deconv=True,
is_batchnorm=True, is_ds=True)``, constructible with zero arguments as ``trainer/trainer.py:337``
does), same attributes, same ``forward(x) -> (final_1, final_2, final_3)`` tuple, and exactly the
reference's ``state_dict`` key names and shapes, so a ``.pth`` written by either loads in the other.

Nothing here executes a ``torch.nn`` layer.  The sub-modules below only *hold* parameters under the
reference's names; all arithmetic runs in ``libunetpp_hip.so`` (see ``engine.py``).  ``depth`` (default
4 = the reference as shipped) extends the topology along the reference's commented-out level-5 lines.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from . import engine

_BASE_WIDTHS = (32, 64, 128, 256, 512)  # models/unet.py:215


class ConvParams(nn.Module):
    """weight [co, ci, k, k] + bias [co], named like nn.Conv2d's (models/unet.py:132,140,191,242)."""

    def __init__(self, cin, cout, k):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = cin, cout, k
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k))
        self.bias = nn.Parameter(torch.empty(cout))
        self.reset_parameters()

    def reset_parameters(self):
        # weights: kaiming-normal fan_in (models/unet.py:165-169); bias keeps torch's default
        # U(-1/sqrt(fan_in), 1/sqrt(fan_in)) because the reference never re-initialises biases.
        fan_in = self.in_channels * self.kernel_size * self.kernel_size
        with torch.no_grad():
            self.weight.normal_(0.0, math.sqrt(2.0 / fan_in))
            bound = 1.0 / math.sqrt(fan_in)
            self.bias.uniform_(-bound, bound)


class DeconvParams(nn.Module):
    """weight [ci, co, 2, 2] + bias [co], named like nn.ConvTranspose2d's (models/unet.py:187)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.in_channels, self.out_channels = cin, cout
        self.weight = nn.Parameter(torch.empty(cin, cout, 2, 2))
        self.bias = nn.Parameter(torch.empty(cout))
        fan_in = cout * 4  # torch's fan_in for a transposed-conv weight: size(1) * receptive field
        with torch.no_grad():
            self.weight.normal_(0.0, math.sqrt(2.0 / fan_in))
            bound = 1.0 / math.sqrt(fan_in)
            self.bias.uniform_(-bound, bound)


class BatchNormParams(nn.Module):
    """gamma/beta + running statistics, named like nn.BatchNorm2d's (models/unet.py:133)."""

    def __init__(self, c, eps=1e-5, momentum=0.1):
        super().__init__()
        self.num_features, self.eps, self.momentum = c, eps, momentum
        self.weight = nn.Parameter(torch.empty(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        with torch.no_grad():
            self.weight.normal_(1.0, 0.02)  # models/unet.py:172-174


class _Slot(nn.Module):
    """Parameter-less placeholder that keeps nn.Sequential's child numbering (ReLU / Upsample slots)."""


def _numbered(*mods):
    holder = nn.Module()
    for i, m in enumerate(mods):
        holder.add_module(str(i), m)
    return holder


class unetConv2(nn.Module):
    """Parameters of models/unet.py:121-156: conv{1,2}.0 = conv, conv{1,2}.1 = BN when is_batchnorm."""

    def __init__(self, in_size, out_size, is_batchnorm, n=2):
        super().__init__()
        self.n, self.is_batchnorm = n, is_batchnorm
        for i in range(1, n + 1):
            mods = [ConvParams(in_size, out_size, 3)]
            if is_batchnorm:
                mods.append(BatchNormParams(out_size))
            mods.append(_Slot())
            self.add_module("conv%d" % i, _numbered(*mods))
            in_size = out_size


class unetUp(nn.Module):
    """Parameters of models/unet.py:182-202: `up` (deconv, or [bilinear, conv1x1]) and the BN-less conv pair."""

    def __init__(self, in_size, out_size, is_deconv, n_concat=2):
        super().__init__()
        self.conv = unetConv2(in_size + (n_concat - 2) * out_size, out_size, False)
        if is_deconv:
            self.up = DeconvParams(in_size, out_size)
        else:
            self.up = _numbered(_Slot(), ConvParams(in_size, out_size, 1))


class UNet_Nested(nn.Module):

    def __init__(self, in_channels=3, n_classes=4, feature_scale=2, is_deconv=True, is_batchnorm=True, is_ds=True,
                 depth=4):
        super().__init__()
        if not 2 <= depth <= len(_BASE_WIDTHS):
            raise ValueError("depth must be in 2..5")
        self.in_channels = in_channels
        self.n_classes = n_classes
        self.feature_scale = feature_scale
        self.is_deconv = is_deconv
        self.is_batchnorm = is_batchnorm
        self.is_ds = is_ds
        self.depth = depth
        filters = [int(x / self.feature_scale) for x in _BASE_WIDTHS]
        if min(filters[:depth]) < 1:
            raise ValueError("feature_scale too large")
        self.filters = filters[:depth]

        cin = in_channels
        for i in range(depth):  # models/unet.py:220-224
            setattr(self, "conv%d0" % i, unetConv2(cin, filters[i], is_batchnorm))
            cin = filters[i]
        for j in range(1, depth):  # :227-239
            for i in range(depth - j):
                setattr(self, "up_concat%d%d" % (i, j), unetUp(filters[i + 1], filters[i], is_deconv, j + 1))
        for j in range(1, depth):  # :242-245
            setattr(self, "final_%d" % j, ConvParams(filters[0], n_classes, 1))
        # Configuration holder only (p and train/eval state are read by the engine; it is never called).
        self.drop_out = nn.Dropout(p=0.4)  # :254
        # Test hook: list of uint8 NHWC keep-masks (one per head) used instead of the in-kernel generator.
        self.dropout_masks = None
        # storage type of the activations and their gradients in HBM: fp32 (reference numerics), or bf16 with fp32
        # accumulation / statistics / parameter gradients (BASELINE configs[3]/[4]); parameters stay fp32 either way
        self.activation_dtype = torch.float32
        # head J when the parameters came from a pruned checkpoint (checkpoint.load_pruned): only the nodes head J needs
        # hold trained weights, so forward() and infer(head > J) refuse to run.  None = every node is usable.
        self.pruned_to = None

    def set_activation_dtype(self, dtype):
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("activation storage is float32 or bfloat16")
        self.activation_dtype = dtype
        return self

    def forward(self, inputs):
        if getattr(self, "pruned_to", None) is not None:
            raise RuntimeError("this model holds a checkpoint pruned to head %d: the other nodes were never loaded; use "
                               "infer(x, head <= %d), or load a full state_dict" % (self.pruned_to, self.pruned_to))
        return engine.run(self, inputs)

    def infer(self, inputs, head=None, ensemble=False):
        """Eval-only inference cut at a deep-supervision head: fp32 ``[B, n_classes, H, W]``, no ``grad_fn``.

        A nested U-Net is trained with one head per decoder column so that it can be cut afterwards: head ``J`` depends
        only on the nodes ``X_ij`` with ``i + j <= J`` (``engine.needed_nodes``).  ``head`` is an int in ``1 .. depth-1``
        (``None`` = the last head).

        * ``ensemble=False`` -- the fast mode: runs only those nodes and that one head.  Every node issues the launches
          of the full graph with the same operands, so the result is bit-identical to ``model(x)[head - 1]`` in eval mode.
        * ``ensemble=True`` -- the accurate mode, the selection models/unet.py:293-298 keeps as comments: the mean of heads
          ``1 .. head``, ``(((s_1 + s_2) + ...) + s_n) / n``, by one kernel that never writes the individual maps.

        Raises ``RuntimeError`` in training mode and ``ValueError`` for any other ``head``; input checks as ``forward``.
        ``validate_step(model, ..., forward=lambda x: (model.infer(x, 1),))`` validates a pruned network."""
        return engine.infer(self, inputs, head, ensemble)

    def infer_mc(self, inputs, head=None, samples=16, p=None, seed=None):
        """Monte-Carlo dropout at deep-supervision head ``head``: ``McMaps(mean, var)``, both fp32
        ``[B, n_classes, H, W]`` without ``grad_fn`` (``.std`` is ``var.sqrt()``).

        The network's one stochastic element is the ``Dropout`` in front of each head's 1x1 convolution; nothing upstream
        of ``X_0J`` is random.  So the pass is ``infer(x, head)``'s -- the same checks (eval mode, ``pruned_to``, BatchNorm
        layers in eval), the same nodes, the same weight-image plan -- and only the head, ``sigmoid(W . dropout(x) + b)``, is
        drawn ``samples`` (2 .. 32) times, in one launch that reads ``X_0J`` once (``ops.head_mc``; a composition of
        ``head_fwd`` launches with the same bits where the channel count or bf16 storage keeps a call off that kernel).
        ``mean`` is the fold ``(((s_0 + s_1) + ...) + s_{K-1}) / K`` and ``var`` the unbiased variance around it: how
        strongly a response depends on which features are present.

        ``p``: drop probability in (0, 1), ``None`` = ``self.drop_out.p``.  ``seed``: ``None`` draws one with
        ``torch.randint`` (so ``torch.manual_seed`` reproduces a call).  Sample ``k`` is the map that ``ops.head_fwd``
        writes for the seed ``seed + 0x632BE59BD9B4E019 * head + 0xD6E8FEB86659FD93 * k (mod 2^64)``.
        ``self.dropout_masks`` (the test hook of the training forward) is ignored: the draws always come from the
        in-kernel generator.  The ensemble mean has no Monte-Carlo form."""
        return engine.infer_mc(self, inputs, head, samples, p, seed)

    def forward_pruned(self, inputs, head=None, ensemble=False):
        """``forward`` of the network cut at deep-supervision head ``head``, connected to autograd as ``forward`` is: only
        the nodes ``X_ij`` with ``i + j <= head`` run (``engine.needed_nodes``), forward and backward, every layer in the
        mode of its own ``training`` flag.  ``head`` as in ``infer`` (``None`` = the last head, the whole network).

        * ``ensemble=False`` -- the tuple of heads ``1 .. head``: the reference's output tuple, shortened.  Head ``j`` draws
          the dropout seed (or takes the mask) ``j - 1`` of the ``depth - 1``, so the same ``torch.manual_seed`` in front of
          ``model(x)`` and ``model.forward_pruned(x, J)`` gives ``model(x)[:J]`` bit for bit.
        * ``ensemble=True`` -- one tensor, the mean of heads ``1 .. head``, the value of ``infer(x, head, ensemble=True)``;
          its backward recomputes the head maps.  The mean has no dropout: with active dropout this raises.

        Parameters outside the cut are not read, get no gradient (``p.grad`` stays as it was) and their BatchNorm buffers
        do not move; ``engine.pruned_parameters(model, head)`` lists the ones inside.  This is how a ``load_pruned`` model
        (``head <= pruned_to``) is trained: ``train_step(..., head=J)``."""
        return engine.run_pruned(self, inputs, head, ensemble)

    def freeze_batchnorm(self, frozen: bool = True, affine: bool = True):
        """The fine-tuning idiom ``for bn in batchnorms: bn.eval()`` in one call: puts every ``BatchNormParams`` into eval
        mode (``frozen=True``) or back into training mode, whatever the mode of the model around them.  A frozen layer
        normalises with its running statistics, updates neither them nor ``num_batches_tracked``, and its backward is one
        streaming launch.  With ``affine=True`` gamma and beta get ``requires_grad = not frozen``; while neither requires
        grad the layer's backward skips their sums and they receive no gradient (``p.grad`` stays ``None``).

        Semantics are torch's: the flags are ordinary ``nn.Module.training`` flags, so a later ``model.train()`` (or
        ``model.eval()``) sets every layer again and un-does the mode part of this call -- call it after ``train()``.  It
        takes effect at the next forward; a captured graph keeps the modes it was captured with.  Returns ``self``."""
        for m in self.modules():
            if isinstance(m, BatchNormParams):
                nn.Module.train(m, not frozen)
                if affine:
                    m.weight.requires_grad_(not frozen)
                    m.bias.requires_grad_(not frozen)
        return self

    # ---- weight-image cache control (ops.PackPlan) ------------------------------------------------
    def freeze_weight_images(self, frozen: bool = True):
        """Serving opt-in: keep the kernels' LDS weight images between passes instead of rebuilding them from the
        parameters every pass (one launch).  Only for weights that really do not change: anything that writes the
        parameters behind the module's back (``p.data`` updates) must be followed by ``invalidate_weight_images()``."""
        plan = engine._plan_of(self)
        plan.frozen = bool(frozen)
        plan.invalidate()
        return self

    def invalidate_weight_images(self):
        plan = self.__dict__.get("_pack_plan")
        if plan is not None:
            plan.invalidate()

    def _apply(self, fn, *args, **kwargs):  # .to() / .cuda() / .float(): new storages
        out = super()._apply(fn, *args, **kwargs)
        self.invalidate_weight_images()
        return out

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.invalidate_weight_images()
        if not getattr(out, "missing_keys", None):   # a full load: every node holds loaded weights again
            self.pruned_to = None
        return out

    def train(self, mode: bool = True):
        self.invalidate_weight_images()
        return super().train(mode)


class double_conv(nn.Module):
    """Parameters of models/unet.py:8-25: `conv` = Sequential(conv, BN, ReLU, conv, BN, ReLU) -> children 0,1,3,4."""

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.conv = _numbered(ConvParams(in_ch, out_ch, 3), BatchNormParams(out_ch), _Slot(),
                              ConvParams(out_ch, out_ch, 3), BatchNormParams(out_ch), _Slot())
        # torch's default initialisation (the reference never re-initialises UNet): BN gamma = 1, conv weights
        # kaiming-uniform(a = sqrt(5)) = U(+-1/sqrt(fan_in)), like the bias
        with torch.no_grad():
            for m in self.conv.children():
                if isinstance(m, BatchNormParams):
                    m.weight.fill_(1.0)
                elif isinstance(m, ConvParams):
                    bound = 1.0 / math.sqrt(m.in_channels * 9)
                    m.weight.uniform_(-bound, bound)


class inconv(nn.Module):
    """models/unet.py:28-35"""

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.conv = double_conv(in_ch, out_ch)


class down(nn.Module):
    """models/unet.py:38-48: mpconv = Sequential(MaxPool2d(2), double_conv)"""

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.mpconv = _numbered(_Slot(), double_conv(in_ch, out_ch))


class up(nn.Module):
    """models/unet.py:51-82, bilinear=True (what UNet builds): `up` has no parameters."""

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.up = _Slot()
        self.conv = double_conv(in_ch, out_ch)


class outconv(nn.Module):
    """models/unet.py:85-92"""

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.conv = ConvParams(in_ch, out_ch, 1)
        with torch.no_grad():
            bound = 1.0 / math.sqrt(in_ch)
            self.conv.weight.uniform_(-bound, bound)


class UNet(nn.Module):
    """Drop-in for the reference's classic U-Net (models/unet.py:94-117): same constructor
    ``UNet(n_classes=5, n_channels=3)``, same ``state_dict`` keys/shapes, ``forward(x) -> sigmoid map [B, n_classes, H, W]``.
    Parameter holders only; the arithmetic runs in libunetpp_hip.so (engine_unet.py).  ``widths`` generalises the
    reference's hard-coded (64, 128, 256, 512, 512)."""

    def __init__(self, n_classes=5, n_channels=3, widths=(64, 128, 256, 512, 512)):
        super().__init__()
        w0, w1, w2, w3, w4 = widths
        self.n_classes, self.n_channels, self.widths = n_classes, n_channels, tuple(widths)
        self.inc = inconv(n_channels, w0)
        self.down1 = down(w0, w1)
        self.down2 = down(w1, w2)
        self.down3 = down(w2, w3)
        self.down4 = down(w3, w4)
        self.up1 = up(w4 + w3, w2)
        self.up2 = up(w2 + w2, w1)
        self.up3 = up(w1 + w1, w0)
        self.up4 = up(w0 + w0, w0)
        self.outc = outconv(w0, n_classes)

    def forward(self, x):
        from . import engine_unet
        return engine_unet.run(self, x)

    freeze_batchnorm = UNet_Nested.freeze_batchnorm
    freeze_weight_images = UNet_Nested.freeze_weight_images
    invalidate_weight_images = UNet_Nested.invalidate_weight_images

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self.invalidate_weight_images()
        return out

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.invalidate_weight_images()
        return out

    def train(self, mode: bool = True):
        self.invalidate_weight_images()
        return super().train(mode)


def count_param(model):
    """models/unet.py:176-180"""
    return sum(p.numel() for p in model.parameters())

"""Weights: seeded generators in the reference's state_dict naming, and the flat blobs the C-ABI parses.

There are no trained checkpoints offline (the reference downloads them at import,
interface.py:29,78), so benchmarks and tests use seeded random weights.  The generators use
numpy's PCG64 so that the golden-fixture script (which loads them into the *reference* modules
with ``load_state_dict(strict=True)``) and the GPU tests reproduce identical tensors.

Checkpoint ingestion (reference format): ``load_checkpoint_state_dict`` accepts the
dict saved by balldetection/helper_balldetection.py:510-529 / uplifting/helper.py:371-391.
"""
import os
import struct
import numpy as np

from . import arch

WASB_MAGIC = b'TTUPWSB1'
UPLIFT_MAGIC = b'TTUPUPL1'


def _np(v):
    if hasattr(v, 'detach'):
        v = v.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(v, dtype=np.float32))


# --------------------------------------------------------------------------- generators
def random_wasb_state_dict(seed=0, planted=False, in_ch=9, head_out=3, eps=0.2, plant_all_heads=False):
    """Seeded WASB/HRNet weights.

    planted=False: Kaiming-scaled noise everywhere, BN running stats randomised so that BN
    folding is exercised (a fresh BatchNorm has mean 0 / var 1).
    planted=True: the same noise scaled by ``eps`` plus an identity path that carries the mean of
    the centre frame's three channels through channel 0 of the full-resolution trunk to head channel 1, so a
    bright blob in the frames produces a dominant heatmap peak (margin >> bf16 rounding) while
    every conv still contributes.  plant_all_heads=True routes the planted trunk channel to EVERY head channel (the 13-keypoint
    table detector of the end-to-end fixtures: all keypoints then follow the blob with the same margin).
    """
    rng = np.random.default_rng(seed)
    sd = {}
    gain = eps if planted else 1.0
    for s in arch.hrnet_convs(in_ch, head_out):
        fan_in = s.cin * s.k * s.k
        sd[s.conv + '.weight'] = (rng.standard_normal((s.cout, s.cin, s.k, s.k)) * np.sqrt(2.0 / fan_in) * gain).astype(np.float32)
        if s.has_bias:
            sd[s.conv + '.bias'] = (rng.standard_normal(s.cout) * 0.1 * gain).astype(np.float32)
        if s.bn:
            damp = 0.5 if s.bn.endswith('bn2') or s.bn.endswith('bn3') else 1.0
            sd[s.bn + '.weight'] = (rng.uniform(0.8, 1.2, s.cout) * damp).astype(np.float32)
            sd[s.bn + '.bias'] = (rng.standard_normal(s.cout) * 0.1 * gain).astype(np.float32)
            sd[s.bn + '.running_mean'] = (rng.standard_normal(s.cout) * 0.1 * gain).astype(np.float32)
            sd[s.bn + '.running_var'] = rng.uniform(0.5, 1.5, s.cout).astype(np.float32)
    if planted:
        def ident_bn(bn):
            sd[bn + '.weight'][0] = 1.0
            sd[bn + '.bias'][0] = 0.0
            sd[bn + '.running_mean'][0] = 0.0
            sd[bn + '.running_var'][0] = 1.0
        p = 'model'
        w = sd[p + '.conv1.weight']; w[0] = 0; w[0, in_ch // 3:2 * in_ch // 3, 1, 1] = 3.0 / in_ch; ident_bn(p + '.bn1')   # centre frame only
        w = sd[p + '.conv2.weight']; w[0] = 0; w[0, 0, 1, 1] = 1.0; ident_bn(p + '.bn2')
        w = sd[p + '.layer1.0.downsample.0.weight']; w[0] = 0; w[0, 0, 0, 0] = 1.0; ident_bn(p + '.layer1.0.downsample.1')
        w = sd[p + '.transition1.0.0.weight']; w[0] = 0; w[0, 0, 1, 1] = 1.0; ident_bn(p + '.transition1.0.1')
        w = sd[p + '.final_layers.0.weight']
        for k in (range(head_out) if plant_all_heads else [1]):
            w[k] *= 0.25; w[k, 0, 0, 0] = 1.0
    return sd


def random_uplift_state_dict(seed=0, size='large', name='connectstage', mode='dynamic', time_rotation='new'):
    """Seeded uplift-transformer weights (xavier-like scale as model.py:22-28,117-121,178-184,243-249;
    biases and LayerNorm randomised so that every term is exercised) of get_model(name, size, mode, time_rotation).
    `time_rotation` changes no weight: 'new' and 'old' of one seed are the same state dict."""
    arch.check_uplift_variant(name, size, mode, time_rotation)
    rng = np.random.default_rng(seed)
    d, depth, heads = arch.UPLIFT_SIZES[size]
    sd = {}
    for k, shape in arch.uplift_variant_schema(name, size, mode):
        if k.endswith('inv_freq'):
            hd = d // heads
            sd[k] = (1.0 / (10000 ** (np.arange(0, hd, 2, dtype=np.float32) / np.float32(hd)))).astype(np.float32)
        elif k.endswith('norm1.weight') or k.endswith('norm2.weight'):
            sd[k] = rng.uniform(0.8, 1.2, shape).astype(np.float32)
        elif k.endswith('.bias'):
            sd[k] = (rng.standard_normal(shape) * 0.05).astype(np.float32)
        elif k == 'cls_token':
            sd[k] = (rng.standard_normal(shape) * 0.1).astype(np.float32)
        else:
            fan_out, fan_in = shape
            a = np.sqrt(6.0 / (fan_in + fan_out))
            sd[k] = rng.uniform(-a, a, shape).astype(np.float32)
    return sd


# --------------------------------------------------------------------------- blobs
def pack_wasb_blob(state_dict, in_ch=9, head_out=3, prefix='model'):
    """Reference-format state_dict -> bytes for ``ttup_wasb_create`` (layout: include/ttup.h)."""
    convs = arch.hrnet_convs(in_ch, head_out, prefix)
    parts = [WASB_MAGIC, struct.pack('<4i', len(convs), in_ch, head_out, 0)]
    for s in convs:
        w = _np(state_dict[s.conv + '.weight'])
        if w.shape != (s.cout, s.cin, s.k, s.k):
            raise ValueError('%s: expected shape %s, got %s' % (s.conv, (s.cout, s.cin, s.k, s.k), w.shape))
        parts.append(struct.pack('<8i', s.cout, s.cin, s.k, s.stride, 1 if s.bn else 0, 1 if s.has_bias else 0, 0, 0))
        parts.append(w.tobytes())
        if s.has_bias:
            parts.append(_np(state_dict[s.conv + '.bias']).tobytes())
        if s.bn:
            for f in ('weight', 'bias', 'running_mean', 'running_var'):
                v = _np(state_dict['%s.%s' % (s.bn, f)])
                if v.shape != (s.cout,):
                    raise ValueError('%s.%s: bad shape %s' % (s.bn, f, v.shape))
                parts.append(v.tobytes())
    return b''.join(parts)


def pack_uplift_blob(state_dict, size='large', name='connectstage', mode='dynamic', time_rotation='new'):
    """Reference-format state_dict -> bytes for ``ttup_uplift_create`` (header and record order: include/ttup.h).
    Raises ValueError naming the first key that is missing, has another variant's shape, or belongs to no layer of this variant."""
    arch.check_uplift_variant(name, size, mode, time_rotation)
    d, depth, heads = arch.UPLIFT_SIZES[size]
    pos, first, second = arch.uplift_variant_layers(name, size, mode)
    schema = arch.uplift_variant_schema(name, size, mode)
    known = {k for k, _ in schema}
    for k in state_dict:
        if k not in known:
            raise ValueError('%s: not a key of uplift variant %s/%s (size %s)' % (k, name, mode, size))
    for k, shape in schema:
        if k not in state_dict:
            raise ValueError('%s: missing from the state dict (uplift variant %s/%s, size %s)' % (k, name, mode, size))
        if _np(state_dict[k]).shape != tuple(shape):
            raise ValueError('%s: expected shape %s, got %s' % (k, shape, _np(state_dict[k]).shape))
    variant = arch.UPLIFT_NAMES.index(name) | arch.UPLIFT_MODES.index(mode) << 4
    parts = [UPLIFT_MAGIC, struct.pack('<8i', d, heads, len(pos), len(first), len(second), 13, variant, arch.UPLIFT_ROTATIONS.index(time_rotation))]
    inv = _np(state_dict[(pos + first + second)[0] + '.attn.rotary_emb.inv_freq'])   # identical in every layer (model.py:51)
    parts += [struct.pack('<i', inv.size), inv.tobytes()]
    # records in state_dict order, except: `embed` (read by multistage only) goes in front of the second stage, and singlestage's
    # position head in front of its rotation head, so that every variant reads ... layers, position head, [embed], second, rotation head
    body = [(k, shape) for k, shape in schema if not k.endswith('inv_freq') and not k.startswith('embed.')]
    if name == 'singlestage':
        body = [e for e in body if not e[0].startswith('rotation_head.')] + [e for e in body if e[0].startswith('rotation_head.')]
    if name == 'multistage':
        at = [e[0] for e in body].index(second[0] + '.attn.qkv.weight')
        body[at:at] = [(k, shape) for k, shape in schema if k.startswith('embed.')]
    for k, shape in body:
        v = _np(state_dict[k])
        parts.append(struct.pack('<i', v.size))
        parts.append(v.tobytes())
    return b''.join(parts)


def load_checkpoint_state_dict(path):
    """Read a reference checkpoint file (torch.save of {'model_state_dict', 'identifier',
    'additional_info'}) -> (state_dict, additional_info).

    A checkpoint folder is user input, so the file is read with ``weights_only=True`` (tensors + plain containers: the default of
    the torch 2.6 the reference pins, and what the reference's detector loaders use, inference_balldetection.py:49).  The
    reference reads the UPLIFTING checkpoint with ``weights_only=False`` (inference_uplifting.py:43) because its
    ``additional_info`` carries the training hyper-parameters, which may hold numpy scalars / dtypes: those are allow-listed on a
    second attempt.  Anything beyond that needs the explicit opt-in ``TTUP_UNSAFE_LOAD=1`` (full unpickling, trusted files only)."""
    import pickle
    import torch
    if os.environ.get('TTUP_UNSAFE_LOAD') == '1':
        d = torch.load(path, map_location='cpu', weights_only=False)
        return d['model_state_dict'], d.get('additional_info', {})
    try:
        d = torch.load(path, map_location='cpu', weights_only=True)
    except pickle.UnpicklingError as first:
        import numpy as np
        allow = [np.dtype, np.ndarray, type(np.dtype('float32')), type(np.dtype('float64')), type(np.dtype('int64')), type(np.dtype('int32')), type(np.dtype('bool'))]
        try:
            from numpy._core.multiarray import scalar, _reconstruct
        except ImportError:                                   # numpy < 2
            from numpy.core.multiarray import scalar, _reconstruct
        allow += [scalar, _reconstruct]
        try:
            with torch.serialization.safe_globals(allow):
                d = torch.load(path, map_location='cpu', weights_only=True)
        except pickle.UnpicklingError:
            raise RuntimeError('checkpoint %s holds pickled objects beyond tensors, containers and numpy scalars (%s); if the file is '
                               'trusted, set TTUP_UNSAFE_LOAD=1 to read it like the reference does (weights_only=False)' % (path, first)) from first
    return d['model_state_dict'], d.get('additional_info', {})


# --------------------------------------------------------------------------- ViTPose-small (balldetection/models/vitpose.py)
VITPOSE_MAGIC = b'TTUPVIT1'
VITPOSE_DIM, VITPOSE_DEPTH, VITPOSE_HEADS, VITPOSE_MLP, VITPOSE_DECONV = 384, 12, 12, 1536, 256
VITPOSE_RESOLUTION = (1152, 640)       # (W, H): balldetection/config.py:82, tabledetection/config.py:76
BN_EPS = 1e-5                          # nn.BatchNorm2d default (topdown_heatmap_simple_head.py:317)


def vitpose_schema(in_ch=9, out_ch=1, resolution=VITPOSE_RESOLUTION, prefix='model'):
    """[(key, shape)] of the reference VitPose wrapper's state_dict (ViTPoseModel under `self.model`) in the order of
    `pack_vitpose_blob`.  resolution (W, H): pos_embed has (W//16)*(H//16)+1 rows (vit.py:215,293)."""
    d, m, f = VITPOSE_DIM, VITPOSE_MLP, VITPOSE_DECONV
    n_pos = (resolution[0] // 16) * (resolution[1] // 16) + 1
    b = prefix + '.backbone.'
    s = [(b + 'pos_embed', (1, n_pos, d)), (b + 'patch_embed.proj.weight', (d, in_ch, 16, 16)), (b + 'patch_embed.proj.bias', (d,))]
    for i in range(VITPOSE_DEPTH):
        p = b + 'blocks.%d.' % i
        s += [(p + 'norm1.weight', (d,)), (p + 'norm1.bias', (d,)), (p + 'attn.qkv.weight', (3 * d, d)), (p + 'attn.qkv.bias', (3 * d,)),
              (p + 'attn.proj.weight', (d, d)), (p + 'attn.proj.bias', (d,)), (p + 'norm2.weight', (d,)), (p + 'norm2.bias', (d,)),
              (p + 'mlp.fc1.weight', (m, d)), (p + 'mlp.fc1.bias', (m,)), (p + 'mlp.fc2.weight', (d, m)), (p + 'mlp.fc2.bias', (d,))]
    s += [(b + 'last_norm.weight', (d,)), (b + 'last_norm.bias', (d,))]
    h = prefix + '.keypoint_head.'
    for i, cin in ((0, d), (3, f)):
        s += [(h + 'deconv_layers.%d.weight' % i, (cin, f, 4, 4))]
        s += [(h + 'deconv_layers.%d.%s' % (i + 1, k), (f,)) for k in ('weight', 'bias', 'running_mean', 'running_var')]
    s += [(h + 'final_layer.weight', (out_ch, f, 1, 1)), (h + 'final_layer.bias', (out_ch,))]
    return s


def random_vitpose_state_dict(seed=0, in_ch=9, out_ch=1, resolution=VITPOSE_RESOLUTION, planted=True):
    """Seeded ViTPose-small weights in the reference's key naming (`model.backbone.*`, `model.keypoint_head.*`).

    Every tensor is noise of a trained-network scale (ViT: trunc-normal 0.02 linears, LayerNorm gains around 1; head: BN running
    statistics randomised so that the BN fold is exercised).  planted=True adds a path that makes the heatmaps PEAKED: token
    channels 0..15 are zero-mean centre-surround filters of the centre frame's patch around a 4x4 grid of sub-centres, blind to
    the taps that reach into the zero padding (a bright blob anywhere in the patch lights up one of them, a smooth background or
    the frame border none), the transformer's residual stream carries them to
    `last_norm`, deconvolution 1 keeps them apart behind its ReLU, deconvolution 2 adds them into its channel 0 and every output
    channel of the final 1x1 conv follows that channel, all with an asymmetric kernel, so each map has one dominant maximum near the
    blob while every weight still contributes."""
    rng = np.random.default_rng(seed)
    sd = {}
    for k, shape in vitpose_schema(in_ch, out_ch, resolution):
        if k.endswith('running_var'):
            v = rng.uniform(0.5, 1.5, shape)
        elif k.endswith('norm1.weight') or k.endswith('norm2.weight') or k.endswith('last_norm.weight') or \
                (k.endswith('.weight') and len(shape) == 1):
            v = rng.uniform(0.8, 1.2, shape)
        elif k.endswith('pos_embed') or k.endswith('.bias') or k.endswith('running_mean'):
            v = rng.standard_normal(shape) * 0.02
        elif k.endswith('patch_embed.proj.weight') or 'deconv_layers' in k or 'final_layer' in k:
            fan_in = shape[1] * shape[2] * shape[3] if 'deconv' not in k else shape[0] * 4
            v = rng.standard_normal(shape) * np.sqrt(1.0 / fan_in) * (0.2 if planted else 1.0)
        else:
            v = rng.standard_normal(shape) * 0.02
        sd[k] = v.astype(np.float32)
    if planted:
        b, h = 'model.backbone.', 'model.keypoint_head.'
        w = sd[b + 'patch_embed.proj.weight']
        frames = slice(in_ch // 3, 2 * in_ch // 3) if in_ch > 3 else slice(0, in_ch)      # the centre frame (or the single frame)
        yy, xx = np.meshgrid(np.arange(16.0), np.arange(16.0), indexing='ij')
        for i in range(16):          # channel i: centre-surround filter around sub-centre i of a 4x4 grid in the patch
            g = np.exp(-((yy - 3.5 - 3.5 * (i // 4)) ** 2 + (xx - 3.5 - 3.5 * (i % 4)) ** 2) / (2 * 2.5 ** 2))
            g[:2] = 0; g[:, :2] = 0                  # the taps that reach into the zero padding (2 px) of the border patches: off
            g[2:, 2:] -= g[2:, 2:].mean()
            w[i] = 0
            w[i, frames] = g * (0.3 / (frames.stop - frames.start))
            sd[b + 'patch_embed.proj.bias'][i] = 0
        k1 = np.array([1.0, 2.0, 4.0, 1.0]) / 4
        w = sd[h + 'deconv_layers.0.weight']
        for i in range(16):          # deconv 1 keeps the 16 sub-centre channels apart (ReLU: a blob in ANY of them is positive) ...
            w[i, i] = np.outer(k1, k1)
        w = sd[h + 'deconv_layers.3.weight']
        for i in range(16):          # ... deconv 2 adds them into channel 0
            w[i, 0] = np.outer(k1, k1)
        for i in (1, 4):
            bn = h + 'deconv_layers.%d.' % i
            n = 16 if i == 1 else 1
            sd[bn + 'weight'][:n], sd[bn + 'bias'][:n], sd[bn + 'running_mean'][:n], sd[bn + 'running_var'][:n] = 1, 0, 0, 1
        sd[h + 'deconv_layers.1.bias'][:16] = -2.0        # threshold: after last_norm a blob's channel is ~10, a background one ~1
        sd[h + 'final_layer.weight'][:, 0] = 1.0
    return sd


def vitpose_fold_head(state_dict, prefix='model'):
    """The head's two ConvTranspose2d(k4,s2,p1) + BN (eval) as four 2x2 sub-convolutions each, BN folded (fp64, rounded once):
    -> [(w (4, cout, 4*cin) float32, b (cout,) float32)] for deconv 1 and 2.  Phase p = 2*py + px produces output pixel
    (2y+py, 2x+px) from input pixels (y+py+dy-1, x+px+dx-1), dy,dx in {0,1}, with reduction index (2*dy+dx)*cin + c and the
    transposed kernel's tap (3-py-2*dy, 3-px-2*dx)."""
    h = prefix + '.keypoint_head.deconv_layers.'
    out = []
    for i in (0, 3):
        w = _np(state_dict[h + '%d.weight' % i]).astype(np.float64)          # (cin, cout, 4, 4)
        g, beta, mu, var = [_np(state_dict[h + '%d.%s' % (i + 1, k)]).astype(np.float64) for k in ('weight', 'bias', 'running_mean', 'running_var')]
        scale = g / np.sqrt(var + BN_EPS)
        cin, cout = w.shape[:2]
        wp = np.empty((4, cout, 4, cin))
        for py in range(2):
            for px in range(2):
                for dy in range(2):
                    for dx in range(2):
                        wp[2 * py + px, :, 2 * dy + dx, :] = w[:, :, 3 - py - 2 * dy, 3 - px - 2 * dx].T * scale[:, None]
        out.append((wp.reshape(4, cout, 4 * cin).astype(np.float32), (beta - mu * scale).astype(np.float32)))
    return out


def pack_vitpose_blob(state_dict, in_ch=9, out_ch=1, prefix='model'):
    """Reference-format VitPose state_dict -> bytes for ``ttup_vitpose_create`` (layout: include/ttup.h)."""
    n_pos = _np(state_dict[prefix + '.backbone.pos_embed']).shape[1]
    schema = vitpose_schema(in_ch, out_ch, prefix=prefix)
    parts = [VITPOSE_MAGIC, struct.pack('<8i', in_ch, out_ch, VITPOSE_DIM, VITPOSE_DEPTH, VITPOSE_HEADS, VITPOSE_MLP, VITPOSE_DECONV, n_pos)]
    for k, shape in schema:
        if 'keypoint_head.deconv_layers' in k:
            continue
        v = _np(state_dict[k])
        if k.endswith('pos_embed'):
            shape = (1, n_pos, VITPOSE_DIM)
        if v.shape != tuple(shape):
            raise ValueError('%s: expected shape %s, got %s' % (k, tuple(shape), v.shape))
        if k.endswith('last_norm.bias'):
            parts.append(v.tobytes())
            for w, b in vitpose_fold_head(state_dict, prefix):
                parts += [w.tobytes(), b.tobytes()]
            continue
        parts.append(v.tobytes())
    return b''.join(parts)

"""The rollout's HIP kernels behind Python objects: the weight packers, the fused policy forwards of both
actor-critic modules, the record / GAE / normalise kernels (HipRolloutKernels) and the inference policies of play and
evaluate.  All of it is the host side of include/go1_rollout.h (learn_abi's structures); nothing here has a CPU or
torch fall-back for a missing kernel.

The plain module's forward is one launch (FusedPolicy: go1_policy_forward in csrc/rollout.hip, the kernels in
csrc/policy_full.h, policy_split.h and policy_actor.hip); the height-map encoder module's is two (FusedEncoderPolicy:
go1_heightmap_encode, csrc/encoder.hip, writes policy_input, then the same go1_policy_forward runs the three heads on
it).
"""
import ctypes as C

import torch
import torch.nn as nn

from . import abi, learn_abi as LA, native
from .actor_critic import CNN_FEATURES, ENC_HIDDEN, ActorCriticCNN
from .rollout_lib import lib


# ----------------------------------------------------------------------------- weight packers
def _pack_linear(lin):
    """nn.Linear -> (weights split and packed for csrc/rollout.hip's 3xF16 MFMA, bias padded to 16).

    Every weight w is split into hi = f16(w) and lo = f16(w - hi).  Packed as 32-byte records
    [n/16][k/32][lane = 16 q + m][hi r = 0..7, lo r = 0..7] of W[16 t + m][32 g + 8 q + r]: lane
    (m, q) of output tile t reads one record per 32-deep K group g -- its A fragments of
    v_mfma_f32_16x16x32_f16 (row m, k = 8 q .. 8 q + 7) for both halves of the split."""
    return _pack_matrix(lin.weight.detach().float(), lin.bias.detach().float())


def _pack_matrix(W, b):
    """_pack_linear for a weight matrix (n, k) and its bias (_pack_conv packs a convolution's filters this way)."""
    n, k = W.shape
    npad, kpad = -(-n // 16) * 16, -(-k // 32) * 32
    Wp = torch.zeros(npad, kpad, device=W.device, dtype=torch.float32)
    Wp[:n, :k] = W
    bp = torch.zeros(npad, device=W.device, dtype=torch.float32)
    bp[:n] = b
    hi = Wp.to(torch.float16)
    lo = (Wp - hi.float()).to(torch.float16)
    # [t, m, g, q, r] -> [t, g, q, m, r], then hi and lo side by side in the last dimension
    def frag(x):
        return x.view(npad // 16, 16, kpad // 32, 4, 8).permute(0, 2, 3, 1, 4)
    return torch.cat([frag(hi), frag(lo)], dim=-1).contiguous(), bp


def _pack_conv(conv):
    """nn.Conv2d (3x3) -> (split packed weights, padded bias) in _pack_linear's record order, the filter of output
    channel oc flattened to the row [oc][ic * 9 + ky * 3 + kx] (K = 9 ic padded to 32)."""
    return _pack_matrix(conv.weight.detach().float().reshape(conv.out_channels, -1), conv.bias.detach().float())


def encoder_layers(ac):
    """The encoder's weight layers in go1_encoder_args.layers order: (Linear, Linear) or (Conv2d, Conv2d, Linear)."""
    m = ac.height_map_encoder.model
    return [m[0], m[3], m[7]] if ac.use_cnn else [m[0], m[2]]


def _rows(x):
    """x detached, as the kernels read a matrix: unit column stride, rows any stride >= the width (a row-strided
    window, such as the velocity env's history, is read in place)."""
    x = x.detach()
    if x.dim() != 2 or x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return x


def _heads_supported(ac, h):
    """Whether go1_policy_forward takes the three heads of `ac` on an input of width h."""
    try:
        shapes = [tuple(m.weight.shape) for m in LA.policy_linears(ac)]
    except (IndexError, AttributeError):
        return False
    npv, na = ac.num_privileged_obs, shapes[6][0]
    # any input width for the default launch (inputs streamed in chunks of 288), as long as the
    # 32-wide groups that hold the latent sit in the last chunk (go1_policy_forward checks the same)
    kin, gl, GL = h + npv, h // 32, -(-(h + npv) // 32)
    g_last = 9 * (-(-GL // 9) - 1)
    return (shapes == LA.policy_shapes(h, npv, na) and 1 <= npv <= 8 and kin <= 16384 and gl >= g_last
            and na <= 16 and isinstance(ac.adaptation_module[1], nn.ELU))


# ----------------------------------------------------------------------------- fused policy forwards
class FusedPolicy:
    """ActorCritic forward for the rollout (act + evaluate) in one HIP kernel
    (csrc/policy_full.h policy_kernel).  Re-pack after every optimiser step."""

    def __init__(self, ac, variant=0):
        self.ac = ac
        self.lib = lib()
        self._forward = self.lib.go1_policy_forward
        self.packed = None
        self.variant = variant  # 0: per-net workgroups of 32 envs, 1: one workgroup of 16 envs (go1_policy_args)
        dev = next(ac.parameters()).device
        self._stream = native.raw_stream_of(dev)
        # workgroups that took the f32 fallback of the range guard (activations beyond f16's range)
        self.overflow = torch.zeros(1, dtype=torch.int32, device=dev)

    @staticmethod
    def supported(ac):
        return _heads_supported(ac, ac.num_obs_history)

    def pack(self):
        ac = self.ac
        mods = LA.policy_linears(ac)
        self.packed = [_pack_linear(m) for m in mods]
        # the unsplit f32 weights for the range guard's fallback (the module's own tensors: an optimiser
        # step updates them in place; the split copies are re-packed)
        self.wf = [m.weight.detach().float().contiguous() for m in mods]
        self.na = mods[6].out_features
        self.np = ac.num_privileged_obs
        self.args = LA.PolicyArgs(num_actions=self.na, num_priv=self.np, overflow=self.overflow.data_ptr())
        for i, (w, b) in enumerate(self.packed):
            self.args.layers[i].w, self.args.layers[i].b = w.data_ptr(), b.data_ptr()
            self.args.layers[i].wf = self.wf[i].data_ptr()

    def forward(self, obs_history, privileged_obs, sample=None, mode=0):
        """-> (mean, value, latent) or, with sample = (rng_seed, rng_step, env_id_offset),
        (mean, value, latent, actions, sigma, log_prob): Normal(mean, std) drawn in-kernel.

        mode (go1_policy_args.mode): 0 act + evaluate; 1 act_student (no critic: value is None, privileged_obs
        may be None); 2 act_teacher (the actor on [history, privileged_obs]; latent is the copy of
        privileged_obs that policy_info["latents"] gets)."""
        if self.packed is None:
            self.pack()
        h = _rows(obs_history)
        p = None
        if privileged_obs is not None:
            p = privileged_obs.detach()
            if not p.is_contiguous():
                p = p.contiguous()
        n = h.shape[0]
        na = self.na
        dev = h.device
        mean = torch.empty(n, na, device=dev)
        value = torch.empty(n, 1, device=dev) if mode == LA.GO1_POLICY_FULL else None
        latent = torch.empty(n, self.np, device=dev)
        a = self.args
        a.variant, a.mode = self.variant, mode
        a.obs_history, a.privileged_obs = h.data_ptr(), p.data_ptr() if p is not None else None
        a.action_mean, a.latent = mean.data_ptr(), latent.data_ptr()
        a.value = value.data_ptr() if value is not None else None
        a.n_envs, a.hist_dim, a.hist_ld = n, h.shape[1], h.stride(0)
        out = (mean, value, latent)
        if sample is not None:
            actions = torch.empty(n, na, device=dev)
            sigma = torch.empty(n, na, device=dev)
            logp = torch.empty(n, device=dev)
            self.std = self.ac.std.detach().contiguous()
            a.std, a.actions, a.action_sigma, a.log_prob = (self.std.data_ptr(), actions.data_ptr(),
                                                            sigma.data_ptr(), logp.data_ptr())
            a.rng_seed, a.rng_step, a.env_id_offset = sample
            out = out + (actions, sigma, logp)
        else:
            a.actions = None
        rc = self._forward(C.byref(a), self._stream())
        if rc:
            native.check(self.lib, rc)
        return out


class FusedEncoderPolicy:
    """ActorCriticCNN forward for the rollout (act + evaluate) in two HIP launches: go1_heightmap_encode writes
    policy_input into a persistent (n, 2 S + E) buffer, go1_policy_forward runs the heads on it (FusedPolicy
    with the buffer as its history).  Re-pack after every optimiser step."""

    def __init__(self, ac):
        self.ac = ac
        self.lib = lib()
        self._encode = self.lib.go1_heightmap_encode
        self.heads = FusedPolicy(ac)
        self.overflow = self.heads.overflow  # one counter: encoder and head workgroups that fell back to f32
        dev = next(ac.parameters()).device
        self._stream = native.raw_stream_of(dev)
        self.packed = None
        self._bufs = {}

    @staticmethod
    def supported(ac):
        if not isinstance(ac, ActorCriticCNN) or not _heads_supported(ac, ac.policy_input_dim):
            return False
        c, x, y = ac.height_map_shape
        return (c == 2 and x <= abi.GO1_MAX_SCAN_X and y <= abi.GO1_MAX_SCAN_Y and ac.cnn_num_embedding <= 512
                and (ac.use_cnn or isinstance(ac.height_map_encoder.model[1], nn.ELU)))

    def pack(self):
        ac = self.ac
        mods = encoder_layers(ac)
        self.packed = [_pack_conv(m) if isinstance(m, nn.Conv2d) else _pack_linear(m) for m in mods]
        self.wf = [m.weight.detach().float().contiguous() for m in mods]
        _, x, y = ac.height_map_shape
        self.n_feat = CNN_FEATURES if ac.use_cnn else ENC_HIDDEN
        self.args = LA.EncoderArgs(num_obs=ac.num_obs, n_scalar=ac.num_scalar, map_x=x, map_y=y,
                                   mode=LA.GO1_ENC_CNN if ac.use_cnn else LA.GO1_ENC_MLP,
                                   n_embed=ac.cnn_num_embedding, n_feat=self.n_feat,
                                   overflow=self.overflow.data_ptr())
        for i, (w, b) in enumerate(self.packed):
            L = self.args.layers[i]
            L.w, L.b, L.wf = w.data_ptr(), b.data_ptr(), self.wf[i].data_ptr()
        self.heads.pack()

    def _buffers(self, n, dev):
        b = self._bufs.get(n)
        if b is None:
            b = self._bufs[n] = (torch.empty(n, self.ac.policy_input_dim, device=dev),
                                 torch.empty(n, self.n_feat, device=dev))
        return b

    def encode(self, obs_history, out=None):
        """policy_input of obs_history (n, H * num_obs), rows any stride >= the width: into `out` (n, 2 S + E), rows
        any stride >= the width, or into the persistent buffer."""
        if self.packed is None:
            self.pack()
        h = _rows(obs_history)
        n = h.shape[0]
        buf, scratch = self._buffers(n, h.device)
        if out is None:
            out = buf
        if out.shape != (n, self.ac.policy_input_dim) or out.stride(1) != 1 or out.dtype != torch.float32:
            raise ValueError("out must be (n, 2 S + E) f32 rows")
        a = self.args
        a.obs_history, a.hist_ld = h.data_ptr(), h.stride(0)
        a.frame_off = h.shape[1] - self.ac.num_obs
        a.scratch, a.policy_input, a.out_ld, a.n_envs = scratch.data_ptr(), out.data_ptr(), out.stride(0), n
        rc = self._encode(C.byref(a), self._stream())
        if rc:
            native.check(self.lib, rc)
        return out

    def forward(self, obs_history, privileged_obs, sample=None, mode=0):
        """FusedPolicy.forward's tuples for the encoder module (the encoder launch is the same in every mode)."""
        return self.heads.forward(self.encode(obs_history), privileged_obs, sample=sample, mode=mode)


# Which encoder modes take FusedEncoderPolicy in the rollout by default: those whose encode + policy launches
# beat the module's torch eager act + evaluate at 4096 envs (tools/encoder_kernel_time.py).
FUSED_DEFAULT = {"mlp": True, "cnn": True}


def fused_policy(ac):
    """What HipRolloutKernels.policy returns for the encoder module: the fused path where it is supported and
    the default for the module's mode (FUSED_DEFAULT), else None (the torch forward)."""
    if FusedEncoderPolicy.supported(ac) and FUSED_DEFAULT["cnn" if ac.use_cnn else "mlp"]:
        return FusedEncoderPolicy(ac)
    return None


# ----------------------------------------------------------------------------- record, GAE, normalise
class HipRolloutKernels:
    """ctypes binding of libgo1_rollout.so; raises when the library or the GPU is missing."""

    def __init__(self):
        self.lib = lib()
        self._record = self.lib.go1_record_transition
        if not torch.cuda.is_available():
            raise native.NativeError("no GPU visible: the rollout kernels have no CPU fallback")

    _SRC = (("obs", "observations"), ("privileged_obs", "privileged_observations"),
            ("obs_history", "observation_histories"), ("actions", "actions"), ("mu", "action_mean"),
            ("sigma", "action_sigma"), ("actions_log_prob", "actions_log_prob"), ("values", "values"),
            ("rewards", "rewards"), ("dones", "dones"), ("time_outs", "time_outs"))

    def record(self, st, step, tr, gamma):
        t = getattr(st, "_tr_struct", None)
        if t is None:
            t = st._tr_struct = LA.Transition()
            st._tr_stream = native.raw_stream_of(st.observations.device)
            t.num_obs, t.num_priv = st.observations.shape[-1], st.privileged_observations.shape[-1]
            t.num_obs_history, t.num_actions = st.observation_histories.shape[-1], st.actions.shape[-1]
            st._tr_dst = [(k, buf) for k, buf in (
                ("st_obs", st.observations), ("st_privileged_obs", st.privileged_observations),
                ("st_obs_history", st.observation_histories), ("st_actions", st.actions), ("st_mu", st.mu),
                ("st_sigma", st.sigma), ("st_actions_log_prob", st.actions_log_prob), ("st_values", st.values),
                ("st_rewards", st.rewards), ("st_dones", st.dones))]
        keep = []
        for k, name in self._SRC:
            v = tr.get(name)
            if v is None:
                setattr(t, k, None)
                continue
            if v.dtype == torch.bool:
                v = v.view(torch.uint8)
            if k == "obs_history" and v.dim() == 2 and v.stride(1) == 1 and v.stride(0) >= v.shape[1]:
                t.obs_history_ld = v.stride(0)  # a row-strided window is copied row by row
            elif not v.is_contiguous():
                v = v.contiguous()
            if k == "obs_history" and v.is_contiguous():
                t.obs_history_ld = 0
            keep.append(v)
            setattr(t, k, v.data_ptr())
        for k, buf in st._tr_dst:
            setattr(t, k, buf[step].data_ptr())
        d = tr.get("time_outs_deferred")  # (flag, pending, dst) device pointers, or None
        t.time_outs_flag, t.time_outs_pending, t.time_outs_dst = d if d is not None else (None, None, None)
        rc = self._record(C.byref(t), st.num_envs, gamma, st._tr_stream())
        if rc:
            native.check(self.lib, rc)
        return keep

    def gae(self, st, last_values, gamma, lam):
        lv = last_values.detach().contiguous()
        native.check(self.lib, self.lib.go1_gae(
            st.rewards.data_ptr(), st.dones.data_ptr(), st.values.data_ptr(), lv.data_ptr(), st.returns.data_ptr(),
            st.advantages.data_ptr(), st.adv_stats.data_ptr(), st.num_transitions_per_env, st.num_envs, gamma, lam,
            native.raw_stream(st.rewards.device)))

    def policy(self, ac):
        """The fused forward of `ac` for the rollout, or None (the module's torch forward)."""
        return FusedPolicy(ac) if FusedPolicy.supported(ac) else fused_policy(ac)

    def normalize(self, st, count):
        native.check(self.lib, self.lib.go1_adv_normalize(st.advantages.data_ptr(), st.adv_stats.data_ptr(),
                                                          float(count), st.advantages.numel(),
                                                          native.raw_stream(st.advantages.device)))


# ----------------------------------------------------------------------------- inference policies
_NO_INFO = {}  # policy(ob) without a policy_info: nothing is copied to the host for it


class InferencePolicy:
    """What fused_inference returns: policy(ob, policy_info={}) -> actions, act_inference / act_expert's signature
    (actor_critic.py:137-152).  `fused` is the FusedPolicy / FusedEncoderPolicy it runs on, or None (the module's
    own act_student / act_teacher)."""

    def __init__(self, ac, fused, teacher, sample):
        self.ac, self.fused, self.teacher = ac, fused, bool(teacher)
        self.mode = LA.GO1_POLICY_TEACHER if teacher else LA.GO1_POLICY_STUDENT
        self.seed = None if sample is None else int(sample)
        self.step = 0  # the Philox counter: one value per call
        self._gen = None

    def pack(self):
        """Re-pack the kernels' weight copies (after the module's parameters changed)."""
        if self.fused is not None:
            self.fused.pack()

    def __call__(self, ob, policy_info=_NO_INFO):
        hist, priv = ob["obs_history"], ob.get("privileged_obs")
        want_info = policy_info is not _NO_INFO
        if self.fused is None:
            with torch.no_grad():
                info = policy_info if want_info else {}
                mean = self.ac.act_teacher(hist, priv, policy_info=info) if self.teacher else \
                    self.ac.act_student(hist, policy_info=info)
                if self.seed is None:
                    return mean
                if self._gen is None:
                    self._gen = torch.Generator(device=mean.device).manual_seed(self.seed)
                return mean + self.ac.std.detach() * torch.randn(mean.shape, generator=self._gen, device=mean.device)
        sample = None
        if self.seed is not None:
            self.step += 1
            sample = (self.seed, self.step, 0)
        out = self.fused.forward(hist, priv if self.teacher else None, sample=sample, mode=self.mode)
        if want_info:  # as the module methods fill it
            policy_info["latents"] = priv if self.teacher else out[2].cpu().numpy()
        return out[0] if sample is None else out[3]


def fused_inference(ac, teacher=False, sample=None):
    """The student (act_inference) or teacher (act_expert) policy of `ac` as a callable
    policy(ob, policy_info={}) -> actions, on the fused HIP kernels (go1_policy_forward in GO1_POLICY_STUDENT /
    GO1_POLICY_TEACHER mode, behind go1_heightmap_encode for the encoder module) where
    HipRolloutKernels.policy(ac) gives one; otherwise (a module on the CPU, an architecture the kernels do not
    take, FUSED_DEFAULT off) on the module's own act_student / act_teacher.

    sample: None returns the action mean, as act_inference / act_expert do; an int seed returns
    Normal(mean, std) draws (in-kernel Philox keyed by the seed, one counter value per call).  The weights are
    packed at the first call; policy.pack() re-packs them after the module's parameters changed."""
    dev = next(ac.parameters()).device
    fused = HipRolloutKernels().policy(ac) if dev.type == "cuda" else None
    return InferencePolicy(ac, fused, teacher, sample)

"""PPO.update on the hand-written HIP update engine (csrc/ppo_update.hip, C ABI include/go1_ppo.h).

`PPOEngine` owns the flat parameter / gradient / Adam-state buffers of an ActorCritic (the module's parameters
become views into the flat parameter buffer, so the state dict, the checkpoints and the fused rollout policy see
every update in place) and runs the mini-batch loop of PPO.update (go1_gym_learn/ppo_cse/ppo.py:98-206):

    per mini-batch:  grad(0) [all-reduce] step(0) grad(1) [all-reduce] step(1)

captured into HIP graphs after the first mini-batch (one graph at world 1; three segments around the two
gradient all-reduces at world > 1, which stay eager RCCL calls).  Hyper-parameters, the adaptive learning rate,
the Adam step counts and the loss sums live on the device: a graph replays correctly after PPO_Args change.

The torch optimizers of ppo.PPO stay the API objects (`PPO.optimizer`, `PPO.adaptation_module_optimizer`):
their per-parameter state entries are views of the engine's Adam state, and a state the caller loaded into them
(`load_state_dict`) is imported before the next update.
"""
import ctypes as C
import os

import torch

from . import learn_abi as LA, native

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GO1_PPO_LIB_OVERRIDE") or os.path.join(HERE, "_build", "libgo1_ppo.so")

NAUX = LA.GO1_PPO_AUX
# state_dict order of the supported ActorCritic, as the engine lays out its flat buffers (go1_ppo.h)
PARAM_NAMES = [f"{seq}.{i}.{k}" for seq, i in LA.POLICY_LINEARS for k in ("weight", "bias")] + ["std"]
N_ADAPT_TENSORS = 2 * LA.N_ADAPT_LINEARS
# the MLP height-map encoder's parameters (actor_critic.ActorCriticCNN): they lead the engine's flat buffers, and the
# adaptation optimizer's slice is encoder + adaptation module (ppo_cse_cnn/ppo.py:170-190 back-propagates the
# adaptation loss through process_obs_history)
ENC_PARAM_NAMES = [f"{seq}.{i}.{k}" for seq, i in LA.ENCODER_LINEARS for k in ("weight", "bias")]
ENC_EMBEDDINGS = (128, 256, 384, 512)
# the CNN height-map encoder's parameters (conv1, conv2, linear): the same place in the flat buffers and slices
CONV_PARAM_NAMES = [f"{seq}.{i}.{k}" for seq, i in LA.CONV_ENCODER_LAYERS for k in ("weight", "bias")]

_lib = None


def load_library(path=None):
    """libgo1_ppo.so, loaded once; NativeError when it is missing or another ABI (no CPU fallback).
    `path`: another build of the same source (tools/ppo_gemm_bench.py compares builds), loaded anew."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    l = native.load_library(path or LIB_PATH, "go1_ppo_abi_version", LA.GO1_PPO_ABI_VERSION, "go1_ppo_last_error",
                            LA.PPO_ARGTYPES)
    sizes = (C.c_int64 * 3)()
    l.go1_ppo_abi_sizes(sizes)
    if sizes[1] != 4 * len(LA.HYPER_FIELDS):  # the hyper block is written as one float32 tensor
        raise native.NativeError(f"go1_ppo_hyper is {sizes[1]} bytes, HYPER_FIELDS names {len(LA.HYPER_FIELDS)} floats")
    if path is None:
        _lib = l
    return l


def _elu(mods):
    return all(isinstance(m, torch.nn.ELU) and m.alpha == 1.0 for m in mods)


def _heads_supported(ac, names, width):
    """The three heads on an input of `width` columns: AC_Args' default widths, ELU, latent 1..8, actions 1..16."""
    a, p, c = ac.adaptation_module, ac.actor_body, ac.critic_body
    if sorted(names) != sorted(PARAM_NAMES) or len(a) != 5 or len(p) != 7 or len(c) != 7:
        return False
    lin = LA.policy_linears(ac)
    npv, na = ac.num_privileged_obs, lin[6].out_features
    ok = [tuple(m.weight.shape) for m in lin] == LA.policy_shapes(width, npv, na)
    acts = [m for seq in (a, p, c) for m in seq if not isinstance(m, torch.nn.Linear)]
    return ok and 1 <= npv <= 8 and 1 <= na <= 16 and _elu(acts)


def supported(ac):
    """The engine's architecture: AC_Args' default widths, ELU, latent 1..8, actions 1..16, no decoder."""
    try:
        return _heads_supported(ac, [n for n, _ in ac.named_parameters()], ac.num_obs_history)
    except AttributeError:
        return False


def encoder_supported(ac):
    """The engine's encoder architecture (go1_ppo_dims.enc_mode 1): actor_critic.ActorCriticCNN with the MLP encoder
    (use_cnn False; map -> 256 -> E, ELU, E in ENC_EMBEDDINGS, a map of 1..4096 values), whole frames in the
    history, and the supported heads on policy_input_dim.  supported() stays False for this module: whether its
    update runs on the engine is ppo.ENGINE_DEFAULT / GO1_PPO_ENCODER_ENGINE's decision."""
    try:
        if ac.use_cnn or not isinstance(ac.recurrent_latent_embedding, torch.nn.Identity):
            return False
        names = [n for n, _ in ac.named_parameters()]
        model, n_map, E = ac.height_map_encoder.model, ac.num_map, ac.cnn_num_embedding
        if len(model) != 4 or sorted(n for n in names if n not in PARAM_NAMES) != sorted(ENC_PARAM_NAMES):
            return False
        shapes = [tuple(model[i].weight.shape) for i in (0, 2)]
        enc = (shapes == [(LA.GO1_PPO_ENC_HIDDEN, n_map), (E, LA.GO1_PPO_ENC_HIDDEN)] and E in ENC_EMBEDDINGS
               and 1 <= n_map <= min(LA.GO1_PPO_ENC_MAX_MAP, ac.num_obs) and _elu([model[1], model[3]])
               and ac.num_obs_history % ac.num_obs == 0 and ac.policy_input_dim == 2 * (ac.num_obs - n_map) + E)
        return enc and _heads_supported(ac, [n for n in names if n in PARAM_NAMES], ac.policy_input_dim)
    except (AttributeError, IndexError, TypeError):
        return False


def conv_encoder_supported(ac):
    """The engine's CNN encoder architecture (go1_ppo_dims.enc_mode 3): actor_critic.ActorCriticCNN with use_cnn on the
    reference's (2, 61, 31) map (the dims do not carry the map's x and y, so no other shape), Conv(2, 16, 3, pad 1)
    ReLU MaxPool(2) Conv(16, 32, 3, pad 1) ReLU MaxPool(2) Flatten Linear(3360, E), E in ENC_EMBEDDINGS, whole
    frames in the history, and the supported heads on policy_input_dim.  Every other shape keeps the torch update."""
    try:
        if not ac.use_cnn or not isinstance(ac.recurrent_latent_embedding, torch.nn.Identity):
            return False
        names = [n for n, _ in ac.named_parameters()]
        model, E = ac.height_map_encoder.model, ac.cnn_num_embedding
        if len(model) != 8 or sorted(n for n in names if n not in PARAM_NAMES) != sorted(CONV_PARAM_NAMES):
            return False
        nn = torch.nn
        kinds = [type(m) for m in model] == [nn.Conv2d, nn.ReLU, nn.MaxPool2d, nn.Conv2d, nn.ReLU, nn.MaxPool2d,
                                             nn.Flatten, nn.Linear]
        convs = all((c.kernel_size, c.stride, c.padding, c.dilation, c.groups, c.padding_mode) ==
                    ((3, 3), (1, 1), (1, 1), (1, 1), 1, "zeros") for c in (model[0], model[3])) if kinds else False
        pools = all((m.kernel_size, m.stride, m.padding, m.dilation, m.ceil_mode) == (2, 2, 0, 1, False)
                    for m in (model[2], model[5])) if kinds else False
        shapes = [tuple(model[i].weight.shape) for i in (0, 3, 7)]
        enc = (kinds and convs and pools and tuple(ac.height_map_shape) == LA.CNN_MAP_SHAPE
               and shapes == [(16, 2, 3, 3), (32, 16, 3, 3), (E, LA.CNN_FEATURES)] and E in ENC_EMBEDDINGS
               and ac.num_map <= ac.num_obs and ac.num_obs_history % ac.num_obs == 0
               and ac.policy_input_dim == 2 * (ac.num_obs - ac.num_map) + E)
        return enc and _heads_supported(ac, [n for n in names if n in PARAM_NAMES], ac.policy_input_dim)
    except (AttributeError, IndexError, TypeError):
        return False


class PPOEngine:
    def __init__(self, alg):
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise native.NativeError("no GPU visible: the PPO update engine has no CPU fallback")
        self.alg = alg
        ac = alg.actor_critic
        self.device = next(ac.parameters()).device
        self.hist, self.priv = ac.num_obs_history, ac.num_privileged_obs
        self.na = ac.actor_body[6].out_features
        # the encoder module (encoder_supported): its parameters lead the flat buffers and the phase-1 slice
        self.enc_dims, enc_names = {}, []
        if encoder_supported(ac) or conv_encoder_supported(ac):
            self.enc_dims = dict(enc_mode=LA.GO1_PPO_ENC_CNN if ac.use_cnn else LA.GO1_PPO_ENC_MLP,
                                 num_obs=ac.num_obs, n_map=ac.num_map, n_embed=ac.cnn_num_embedding)
            enc_names = CONV_PARAM_NAMES if ac.use_cnn else ENC_PARAM_NAMES
        self.names = enc_names + PARAM_NAMES
        self.n_adapt_tensors = N_ADAPT_TENSORS + len(enc_names)
        self._stream = native.raw_stream_of(self.device)
        dims = LA.PPODims(hist=self.hist, priv=self.priv, actions=self.na, mb=1, rows=1, **self.enc_dims)
        tot, ad = C.c_int64(), C.c_int64()
        native.check(self.lib, self.lib.go1_ppo_param_count(C.byref(dims), C.byref(tot), C.byref(ad)))
        self.n_total, self.n_adapt = tot.value, ad.value
        dev = self.device
        sd = dict(ac.named_parameters())
        self.offsets = {}
        off = 0
        for name in self.names:
            self.offsets[name] = off
            off += sd[name].numel()
        if off != self.n_total or self.offsets[self.names[self.n_adapt_tensors]] != self.n_adapt:
            raise native.NativeError("PPO engine: parameter layout mismatch between the module and go1_ppo.h")
        # flat buffers; the module's parameters become views into `params`
        self.params = torch.empty(self.n_total, dtype=torch.float32, device=dev)
        for name in self.names:
            p, o = sd[name], self.offsets[name]
            self.params[o:o + p.numel()].copy_(p.detach().reshape(-1))
            p.data = self.params[o:o + p.numel()].view_as(p)
        self.grads = torch.zeros(NAUX + self.n_total, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(self.n_total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        self.ad_exp_avg = torch.zeros(self.n_adapt, dtype=torch.float32, device=dev)
        self.ad_exp_avg_sq = torch.zeros_like(self.ad_exp_avg)
        self.steps = torch.zeros(2, dtype=torch.float32, device=dev)
        self.lr = torch.tensor([alg.learning_rate], dtype=torch.float64, device=dev)
        self.hyper = torch.zeros(len(LA.HYPER_FIELDS), dtype=torch.float32, device=dev)
        self.losses = torch.zeros(4, dtype=torch.float64, device=dev)
        self._hyper_host = None
        self._lr_host = float(alg.learning_rate)
        self.work = None
        self.dims = None
        self.bufs = LA.PPOBufs()
        self.graphs = None
        self._graph_key = None
        self.idx = self._draw = self._side = None  # mini-batch rows, the unused sample's arguments, capture stream
        self._import_optimizer_state()
        self._install_optimizer_views()

    # ------------------------------------------------------------------ helpers
    def _param_list(self, adaptation_only=False):
        sd = dict(self.alg.actor_critic.named_parameters())
        names = self.names[:self.n_adapt_tensors] if adaptation_only else self.names
        return [(n, sd[n]) for n in names]

    def _views(self, flat, adaptation_only=False):
        out = {}
        for name, p in self._param_list(adaptation_only):
            o = self.offsets[name]
            out[name] = flat[o:o + p.numel()].view_as(p)
        return out

    def _install_optimizer_views(self):
        """torch.optim.Adam-shaped state entries that are views of the engine's state (state_dict works)."""
        alg = self.alg
        for opt, (m1, m2), k, ad in ((alg.optimizer, (self.exp_avg, self.exp_avg_sq), 0, False),
                                     (alg.adaptation_module_optimizer, (self.ad_exp_avg, self.ad_exp_avg_sq), 1, True)):
            v1, v2 = self._views(m1, ad), self._views(m2, ad)
            for name, p in self._param_list(ad):
                opt.state[p] = {"step": self.steps[k], "exp_avg": v1[name], "exp_avg_sq": v2[name]}
        self._state_ptrs = self._optimizer_state_ptrs()

    def release_optimizer_state(self):
        """Give every parameter's optimizer state its own tensors again (copies of the engine's), before a torch
        optimizer steps them: the views share one `step` per optimizer, which a torch Adam would increment once
        per parameter.  The next engine update imports the state back (_sync_external_changes)."""
        alg = self.alg
        for opt, (m1, m2), k, ad in ((alg.optimizer, (self.exp_avg, self.exp_avg_sq), 0, False),
                                     (alg.adaptation_module_optimizer, (self.ad_exp_avg, self.ad_exp_avg_sq), 1, True)):
            g = opt.defaults
            on_dev = bool(g.get("fused") or g.get("capturable"))
            v1, v2 = self._views(m1, ad), self._views(m2, ad)
            for name, p in self._param_list(ad):
                step = self.steps[k].detach().clone()
                opt.state[p] = {"step": step if on_dev else step.cpu(), "exp_avg": v1[name].clone(),
                                "exp_avg_sq": v2[name].clone()}
        self._state_ptrs = None

    def _optimizer_state_ptrs(self):
        alg = self.alg
        return tuple(t.data_ptr() for opt in (alg.optimizer, alg.adaptation_module_optimizer)
                     for s in opt.state.values() for t in s.values() if isinstance(t, torch.Tensor))

    def _import_optimizer_state(self):
        """Copy torch-optimizer state (a previous torch-path update or load_state_dict) into the flat buffers."""
        alg = self.alg
        for opt, (m1, m2), k, ad in ((alg.optimizer, (self.exp_avg, self.exp_avg_sq), 0, False),
                                     (alg.adaptation_module_optimizer, (self.ad_exp_avg, self.ad_exp_avg_sq), 1, True)):
            v1, v2 = self._views(m1, ad), self._views(m2, ad)
            for name, p in self._param_list(ad):
                st = opt.state.get(p)
                if not st:
                    continue
                if "exp_avg" in st and st["exp_avg"].data_ptr() != v1[name].data_ptr():
                    v1[name].copy_(st["exp_avg"].detach().reshape(v1[name].shape))
                    v2[name].copy_(st["exp_avg_sq"].detach().reshape(v2[name].shape))
                if "step" in st:
                    self.steps[k].copy_(torch.as_tensor(st["step"], dtype=torch.float32).reshape(()))

    def _sync_external_changes(self):
        """Parameters or optimizer state replaced outside the engine since the last update."""
        ac = self.alg.actor_critic
        relink = False
        for name, p in self._param_list():
            o = self.offsets[name]
            if p.data_ptr() != self.params.data_ptr() + 4 * o:
                self.params[o:o + p.numel()].copy_(p.detach().reshape(-1))
                p.data = self.params[o:o + p.numel()].view_as(p)
                relink = True
        if self._optimizer_state_ptrs() != self._state_ptrs:
            self._import_optimizer_state()
            self._install_optimizer_views()
        return ac

    def _write_hyper(self, A, world):
        vals = (A.clip_param, A.value_loss_coef, A.entropy_coef, A.max_grad_norm,
                A.desired_kl if (A.desired_kl is not None and A.schedule == "adaptive") else 0.0,
                1.0 if A.use_clipped_value_loss else 0.0, 1.0 if A.selective_adaptation_module_loss else 0.0,
                0.9, 0.999, 1e-8, float(world), A.adaptation_module_learning_rate)
        vals = tuple(float(v) for v in vals)
        if vals != self._hyper_host:
            self.hyper.copy_(torch.tensor(vals, dtype=torch.float32))
            self._hyper_host = vals
        # Adam betas / eps from the torch optimizers' param groups (the reference's defaults)
        g = self.alg.optimizer.param_groups[0]
        b1, b2 = g.get("betas", (0.9, 0.999))
        eps = g.get("eps", 1e-8)
        if (b1, b2, eps) != (0.9, 0.999, 1e-8):
            v = list(vals)
            v[7:10] = [float(b1), float(b2), float(eps)]
            self.hyper.copy_(torch.tensor(v, dtype=torch.float32))
            self._hyper_host = tuple(v)

    def _bind(self, st, mb):
        rows = st.num_envs * st.num_transitions_per_env
        dims = LA.PPODims(hist=self.hist, priv=self.priv, actions=self.na, mb=mb, rows=rows, **self.enc_dims)
        nb = C.c_int64()
        native.check(self.lib, self.lib.go1_ppo_workspace_bytes(C.byref(dims), C.byref(nb)))
        if self.work is None or self.work.numel() < nb.value:
            self.work = torch.zeros(nb.value + 256, dtype=torch.uint8, device=self.device)
            self.graphs = None
        self.dims = dims
        b = self.bufs
        hist = st.observation_histories.flatten(0, 1)
        if hist.stride(1) != 1:
            hist = hist.contiguous()
        self._flat = [hist] + [x.flatten(0, 1).contiguous() for x in (
            st.privileged_observations, st.actions, st.values, st.advantages, st.returns, st.actions_log_prob, st.mu,
            st.sigma)]
        b.obs_history, b.hist_ld = hist.data_ptr(), hist.stride(0)
        for k, t in zip(("privileged_obs", "actions", "values", "advantages", "returns", "actions_log_prob", "mu",
                         "sigma"), self._flat[1:]):
            setattr(b, k, t.data_ptr())
        if self.idx is None or self.idx.numel() != mb:
            self.idx = torch.zeros(mb, dtype=torch.int64, device=self.device)
            self.graphs = None
        b.idx = self.idx.data_ptr()
        for k in ("params", "grads", "exp_avg", "exp_avg_sq", "ad_exp_avg", "ad_exp_avg_sq", "steps", "lr", "hyper",
                  "losses"):
            setattr(b, k, getattr(self, k).data_ptr())
        base = self.work.data_ptr()
        b.work = (base + 255) // 256 * 256
        return (mb, rows) + tuple(t.data_ptr() for t in self._flat)

    # ------------------------------------------------------------------ the C-ABI calls
    def pack(self):
        native.check(self.lib, self.lib.go1_ppo_pack(C.byref(self.dims), C.byref(self.bufs), self._stream()))

    def grad(self, phase):
        native.check(self.lib, self.lib.go1_ppo_grad(C.byref(self.dims), C.byref(self.bufs), phase, self._stream()))

    def step(self, phase):
        native.check(self.lib, self.lib.go1_ppo_step(C.byref(self.dims), C.byref(self.bufs), phase, self._stream()))

    def _allreduce(self, n):
        torch.distributed.all_reduce(self.grads[:NAUX + n])

    def _segments(self, world, split):
        """The mini-batch as ("hip", fn) work segments and ("ar", fn) gradient all-reduces between them."""
        if world == 1 and not split:
            return [("hip", lambda: (self.grad(0), self.step(0), self.grad(1), self.step(1)))]
        segs = [("hip", lambda: self.grad(0))]
        if world > 1:
            segs.append(("ar", lambda: self._allreduce(self.n_total)))
        segs.append(("hip", lambda: (self.step(0), self.grad(1))))
        if world > 1:
            segs.append(("ar", lambda: self._allreduce(self.n_adapt)))
        segs.append(("hip", lambda: self.step(1)))
        return segs

    # ------------------------------------------------------------------ PPO.update
    def update(self, A, num_mini_batches, num_epochs, world, use_graph=True, split=False):
        """The mini-batch loop of PPO.update; returns the four loss sums (value, surrogate, adaptation,
        adaptation test) over the mini-batches and the final learning rate."""
        alg = self.alg
        st = alg.storage
        self._sync_external_changes()
        if float(alg.learning_rate) != self._lr_host:  # the caller changed the rate between updates
            self.lr.fill_(float(alg.learning_rate))
        batch = st.num_envs * st.num_transitions_per_env
        mb = batch // num_mini_batches
        key = self._bind(st, mb)
        self._write_hyper(A, world)
        # the f16 fragment images from the current weights, every update: an in-place write to the parameters
        # (load_state_dict, a torch-path update, std.data edits) keeps their storage, so no pointer check sees it
        self.pack()
        self.losses.zero_()
        indices = torch.randperm(num_mini_batches * mb, device=self.device)  # mini_batch_generator's draw
        draw = self._draw
        if draw is None or draw[0].shape != (mb, self.na):
            self._draw = draw = (torch.zeros(mb, self.na, device=self.device),
                                 torch.ones(mb, self.na, device=self.device))
        segs = self._segments(world, split)
        gkey = (key, world, split, self.work.data_ptr(), self.idx.data_ptr())
        if self.graphs is not None and self._graph_key != gkey:
            self.graphs = None
        for _ in range(num_epochs):
            for i in range(num_mini_batches):
                self.idx.copy_(indices[i * mb:(i + 1) * mb])
                torch.normal(*draw)  # ac.act's unused sample (ppo.py:110): the reference's torch RNG consumption
                if self.graphs is not None:
                    for kind, g in self.graphs:
                        g() if kind == "ar" else g.replay()
                    continue
                for _, fn in segs:
                    fn()
                if use_graph:
                    self._capture(segs, gkey)
        out = self.losses.cpu().tolist()
        lr = float(self.lr.item())
        self._lr_host = lr
        return out, lr

    def _capture(self, segs, gkey):
        """Capture the HIP segments (all-reduces stay eager callables between them), once the kernels are loaded."""
        torch.cuda.synchronize(self.device)
        side = self._side
        if side is None:
            side = self._side = torch.cuda.Stream(self.device)
        graphs = []
        for kind, fn in segs:
            if kind == "ar":
                graphs.append((kind, fn))
                continue
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                fn()
            graphs.append((kind, g))
        self.graphs = graphs
        self._graph_key = gkey

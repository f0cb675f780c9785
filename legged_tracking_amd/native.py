"""Thin host binding of the HIP C ABI (include/go1_mi355x.h) over PyTorch-ROCm tensors.

torch provides device memory and the stream; every computation of the step runs
in the HIP library legged_tracking_amd/_build/libgo1_mi355x.so.  If that library
is missing or the GPU is absent this module raises -- there is no CPU fallback.

It also holds what every binding of this package shares: load_library / check, the raw-stream partial, NativeHandle
for the step handles, and the shim of the after-step add-ons (render.py, trace.py, plan.py, randomize.py):
load_addon, dense, need_gpu and AddOn.
"""
import ctypes as C
import functools
import os

import numpy as np
import torch

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GO1_LIB_OVERRIDE") or os.path.join(HERE, "_build", "libgo1_mi355x.so")
_lib = None


class NativeError(RuntimeError):
    pass


def load_library(path, version_fn, version, error_fn, argtypes):
    """dlopen a HIP library of this package, set its prototypes and check its ABI version (fails loudly;
    build with __graft_entry__.build()).  `argtypes` is {function: [ctypes types]}; the loaded library
    carries `last_error` for check()."""
    if not os.path.exists(path):
        raise NativeError(f"HIP extension missing: {path} (run python -c 'import __graft_entry__ as g; g.build()')")
    l = C.CDLL(path)
    getattr(l, version_fn).restype = C.c_int
    l.last_error = getattr(l, error_fn)
    l.last_error.restype = C.c_char_p
    for name, types in argtypes.items():
        getattr(l, name).argtypes = types
    if getattr(l, version_fn)() != version:
        raise NativeError(f"ABI version mismatch: {path} is not version {version} ({version_fn})")
    return l


def check(l, rc):
    if rc != 0:
        raise NativeError(l.last_error().decode())


def raw_stream_of(device):
    """A callable returning the hipStream_t (as an int) of torch's current stream on `device` (no index: the
    device current now).  A partial of the C function, because the per-step paths call it."""
    index = torch.device(device).index
    return functools.partial(torch._C._cuda_getCurrentRawStream,
                             index if index is not None else torch.cuda.current_device())


def raw_stream(device="cuda"):
    """The caller's current raw stream on `device`, for a call off the per-step path."""
    return raw_stream_of(device)()


# ---------------------------------------------------------------------------- after-step add-ons
_addons = {}


def load_addon(path, prefix, version, argtypes, sizes=None):
    """The add-on library at `path`, loaded once per path: load_library with <prefix>_abi_version and
    <prefix>_last_error, then <prefix>_abi_sizes against `sizes`, the list the binding's ctypes mirrors give."""
    l = _addons.get(path)
    if l is None:
        l = load_library(path, prefix + "_abi_version", version, prefix + "_last_error", argtypes)
        if sizes is not None:
            out = (C.c_int64 * len(sizes))()
            getattr(l, prefix + "_abi_sizes")(out)
            if list(out) != list(sizes):
                raise NativeError(f"{path}: {prefix}_abi_sizes gives {list(out)}, the binding has {list(sizes)}")
        _addons[path] = l
    return l


def dense(name, t, shape, dtypes, device=None, what=None):
    """The data pointer of `t`, a contiguous tensor of `shape` and one of `dtypes`, on `device` where one is given;
    NativeError otherwise.  An int `shape` is an element count: the flat form, which an (n,) and an (n, 1) plane
    both meet.  `what` words the failure ("<name> must be <what>") for a caller that has a wording of its own."""
    flat = isinstance(shape, int)
    if t is None or (t.numel() != shape if flat else tuple(t.shape) != tuple(shape)) or t.dtype not in dtypes or \
            not t.is_contiguous() or (device is not None and t.device != device):
        if what is None:
            what = "a contiguous %s %s tensor" % (f"({shape},) or ({shape}, 1)" if flat else tuple(shape),
                                                 " / ".join(map(str, dtypes)))
            if device is not None:
                what += f" on {device}"
        raise NativeError(f"{name} must be {what}")
    return t.data_ptr()


def need_gpu(device, what):
    if device.type != "cuda":
        raise NativeError(f"no GPU visible: the MI355X {what} has no CPU fallback")


class AddOn:
    """Base of the add-ons' launch owners (render.Renderer, trace.TraceBuffers, plan.PlanBuffers,
    randomize.DrBuffers): the device, the caller's current raw stream on it and the return-code check.  One on a CPU
    device can be built (the injected test backends do that) and loads nothing; only its launch raises."""
    WHAT = "add-on"

    def _open(self, device, lib):
        """`lib` is the module's loader, called for a GPU device only."""
        self.device = torch.device(device)
        self._lib = None
        if self.device.type == "cuda":
            self._lib = lib()
            self._stream = raw_stream_of(self.device)

    def _need_gpu(self):
        need_gpu(self.device, self.WHAT)

    def _launch(self, fn, *args):
        """Library function `fn`(*args, stream) on the caller's current stream."""
        rc = getattr(self._lib, fn)(*args, self._stream())
        if rc:
            check(self._lib, rc)


_ARGTYPES = {
    "go1_create": [C.POINTER(abi.Go1Config), C.POINTER(C.c_void_p)],
    "go1_bind": [C.c_void_p, C.POINTER(abi.Go1State), C.POINTER(abi.Go1Plane)],
    "go1_set_terrain": [C.c_void_p, C.POINTER(abi.Go1Terrain)],
    "go1_step": [C.c_void_p, C.POINTER(abi.Go1StepArgs), C.c_void_p],
    "go1_reset_envs": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p],
    "go1_reset_idx": [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p],
    "go1_sync_time_outs": [C.c_void_p, C.c_void_p],
    "go1_time_outs_pending": [C.c_void_p, C.POINTER(C.c_int64)],
    "go1_actuator_net": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p],
    "go1_destroy": [C.c_void_p],
    "go1_specialize": [C.c_void_p, C.c_int],
    "go1_is_specialized": [C.c_void_p],
    "go1_scan_mode": [C.c_void_p, C.c_int],
    "go1_is_streamed": [C.c_void_p],
    "go1_tunnel_tiles": [C.POINTER(abi.Go1TunnelParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "go1_tunnel_generate": [C.POINTER(abi.Go1TunnelSpec), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
}


def lib():
    """The HIP step library, loaded once."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, "go1_abi_version", abi.GO1_ABI_VERSION, "go1_last_error", _ARGTYPES)
    return _lib


class NativeHandle:
    """Base of the handle owners (Go1Native, velocity.VelNative): the device, the caller's current raw stream
    on it, reset_idx's id conversion and close / __del__ through the library's destroy function."""
    WHAT = "step"

    def _open(self, device, l, destroy):
        if not torch.cuda.is_available():
            raise NativeError(f"no GPU visible: the MI355X {self.WHAT} has no CPU fallback")
        self.device = torch.device(device)
        self.h = C.c_void_p()
        self._lib, self._destroy = l, destroy
        self._stream = raw_stream_of(self.device)

    def _check(self, rc):
        check(self._lib, rc)

    def _ids(self, env_ids):
        """Local env ids (any integer tensor or list) as a contiguous int32 tensor on the device; the caller
        keeps it alive until the stream passes it."""
        return torch.as_tensor(env_ids, device=self.device).to(torch.int32).flatten().contiguous()

    def close(self):
        if self.h:
            self._destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pyramid_params(c):
    return abi.Go1PyramidParams(num_x=int(c.pyramid_num_x), num_y=int(c.pyramid_num_y),
                                var_x=float(c.pyramid_var_x), var_y=float(c.pyramid_var_y),
                                length_min=float(c.pyramid_length_min), length_max=float(c.pyramid_length_max),
                                height_min=float(c.pyramid_height_min), height_max=float(c.pyramid_height_max))


def tunnel_tiles(cfg_terrain, layout, seed, device):
    """Tunnel tiles of cfg_terrain.terrain_type generated on the GPU: the tiles the reference's
    Terrain(cfg) builds after np.random.seed(seed), as a (rows, cols, 2, tile_x, tile_y) f32
    tensor on `device` (tunnel.py:51-217; tunnel_fn.py:99-163 single_path, :44-97 narrow_path,
    :546-581 random_pyramid).  single_path goes through go1_tunnel_tiles, the other two through
    go1_tunnel_generate.  ValueError before any device work for what the generators reject."""
    from . import terrain as T
    t = cfg_terrain
    rows, cols = int(t.num_rows), int(t.num_cols)
    if not 0 <= int(seed) < 2 ** 32:
        raise ValueError("seed must be in [0, 2**32) (numpy RandomState)")
    if t.terrain_type not in T.KINDS:
        raise ValueError(f"terrain_type {t.terrain_type!r}: the generator builds {', '.join(T.KINDS)}")
    kind = T.KINDS.index(t.terrain_type)
    pyramid = kind == abi.GO1_TUNNEL_RANDOM_PYRAMID
    if pyramid:
        T.check_pyramid_params(t)
    p = abi.Go1TunnelParams(num_rows=rows, num_cols=cols, tile_x=layout.tile_x, tile_y=layout.tile_y,
                            sub_x=layout.sub_shape[0], sub_y=layout.sub_shape[1], seed=int(seed),
                            horizontal_scale=float(t.horizontal_scale), vertical_scale=float(t.vertical_scale),
                            ceiling_height=float(t.ceiling_height),
                            # (the reference's default Cfg has neither: train.py sets them for single_path)
                            p_flat=0.0 if pyramid else float(t.p_flat), p_double=0.0 if pyramid else float(t.p_double))
    ex = np.ascontiguousarray(layout.extents, np.int32)
    span = np.stack([ex[:, 1] - ex[:, 0], ex[:, 3] - ex[:, 2]], 1)
    bad = np.nonzero((span != np.array([layout.sub_shape[1], layout.sub_shape[0]])).any(1))[0]
    if bad.size:  # the reference's tile[0, sx:ex, sy:ey] = top.T raises on this mismatch (tunnel.py:193-196)
        k = int(bad[0])
        raise ValueError(f"sub-terrain {k}: tunnel extent {tuple(span[k])} does not match the sub-terrain shape "
                         f"{(layout.sub_shape[1], layout.sub_shape[0])} (could not broadcast)")
    ext = torch.as_tensor(ex).to(device)
    rec_w = abi.GO1_TUNNEL_REC if kind == abi.GO1_TUNNEL_SINGLE_PATH else abi.GO1_TUNNEL_SPEC_REC
    rec = torch.empty((rows * cols, rec_w), dtype=torch.float64, device=device)
    tiles = torch.empty((rows, cols, 2, layout.tile_x, layout.tile_y), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        stream = raw_stream()
        if kind == abi.GO1_TUNNEL_SINGLE_PATH:
            rc = lib().go1_tunnel_tiles(C.byref(p), ext.data_ptr(), rec.data_ptr(), tiles.data_ptr(), stream)
        else:
            spec = abi.Go1TunnelSpec(base=p, kind=kind)
            if pyramid:
                spec.top, spec.bottom = _pyramid_params(t.top), _pyramid_params(t.bottom)
            rc = lib().go1_tunnel_generate(C.byref(spec), ext.data_ptr(), rec.data_ptr(), tiles.data_ptr(), stream)
        check(lib(), rc)
    torch.cuda.current_stream(device).synchronize()  # ext / rec are freed on return
    return tiles


class StateTensors:
    """go1_state planes as torch tensors on the device (SoA, row-major (n, width))."""

    def __init__(self, n, device, cfg):
        self.n = n
        self.t = {}
        for name, w, dt in abi.state_spec(cfg):
            self.t[name] = torch.zeros((n, w), dtype=torch.float32 if dt == "f32" else torch.int32, device=device)

    def struct(self):
        return abi.Go1State(**{k: v.data_ptr() for k, v in self.t.items()})

    def __getitem__(self, k):
        return self.t[k]

    def load(self, arrays: dict):
        for k, v in arrays.items():
            if k in self.t:
                self.t[k].copy_(torch.as_tensor(np.asarray(v)).reshape(self.t[k].shape).to(self.t[k].dtype))

    def numpy(self):
        return {k: v.cpu().numpy() for k, v in self.t.items()}


OUT_KEYS = ("obs", "priv", "rew", "reset", "time_out")


class Go1Native(NativeHandle):
    """Owns one go1_handle and the device buffers the C ABI writes."""

    def __init__(self, cfg: abi.Go1Config, device="cuda:0"):
        self._open(device, lib(), lib().go1_destroy)
        self.cfg = cfg
        self.n = n = cfg.n_envs
        with torch.cuda.device(self.device):
            self._check(self._lib.go1_create(C.byref(cfg), C.byref(self.h)))
            self.state = StateTensors(n, self.device, cfg)
            self.bind(self.state)
            dev = self.device
            self.obs = torch.zeros((n, cfg.num_obs), device=dev)
            self.priv = torch.zeros((n, abi.GO1_NUM_PRIV), device=dev)
            self.rew = torch.zeros(n, device=dev)
            self.reset = torch.zeros(n, dtype=torch.bool, device=dev)
            self.time_out = torch.zeros(n, dtype=torch.bool, device=dev)
            self.extras_time_outs = torch.zeros(n, dtype=torch.bool, device=dev)
            self.contact_forces = torch.zeros((n, 17, 3), device=dev)
        self._terrain_keep = None
        self._args = None
        self._lib_step = self._lib.go1_step

    def bind(self, state):
        """go1_bind the planes of `state` (StateTensors or {name: tensor}); the library checks their
        shapes, dtypes and strides and raises NativeError for anything but dense (n_envs, width)."""
        t = state.t if hasattr(state, "t") else state
        s = abi.Go1State(**{k: t[k].data_ptr() for k, _ in abi.Go1State._fields_})
        self._check(self._lib.go1_bind(self.h, C.byref(s), abi.plane_descs(abi.Go1State._fields_, t)))

    def set_terrain(self, tiles, env_tile, env_terrain_origin, env_origins):
        d = self.device
        if isinstance(tiles, torch.Tensor):  # device-generated tiles (tunnel_tiles)
            tiles = tiles.to(d, torch.float32).contiguous()
        else:
            tiles = torch.as_tensor(np.ascontiguousarray(tiles, np.float32)).to(d)
        t = [tiles,
             torch.as_tensor(np.ascontiguousarray(env_tile, np.int32)).to(d),
             torch.as_tensor(np.ascontiguousarray(env_terrain_origin, np.float32)).to(d),
             torch.as_tensor(np.ascontiguousarray(env_origins, np.float32)).to(d)]
        if self.cfg.terrain_kind == 1 and tuple(t[0].shape[1:]) != (2, self.cfg.hf_nx, self.cfg.hf_ny):
            # the kernels take the tile shape from the config: another shape would be mis-indexed without any error
            raise NativeError(f"terrain tiles are {tuple(t[0].shape)}, the handle's config indexes them as "
                              f"(n_tiles, 2, {self.cfg.hf_nx}, {self.cfg.hf_ny}) (go1_config.hf_nx / hf_ny)")
        self._terrain_keep = t
        s = abi.Go1Terrain(tiles=t[0].data_ptr(), env_tile=t[1].data_ptr(), env_terrain_origin=t[2].data_ptr(),
                           env_origins=t[3].data_ptr(), n_tiles=int(t[0].shape[0]))
        self._check(self._lib.go1_set_terrain(self.h, C.byref(s)))

    # ------------------------------------------------------------------ argument checks shared by the step forms
    def _new_args(self):
        a = abi.Go1StepArgs()
        a.extras_time_outs = self.extras_time_outs.data_ptr()
        a._consts = None  # key of the gravity / reward-scale values the block holds
        return a

    def _check_actions(self, a, actions):
        if actions.dtype != torch.float32 or actions.shape != (self.n, 12) or not actions.is_contiguous() or \
                actions.device != self.device:
            raise NativeError("actions must be a contiguous (n_envs, 12) float32 tensor on the env's device")
        a.actions = actions.data_ptr()

    def _check_out(self, a, out):
        """Output pointers: the buffers of `out` (checked), the handle's own for keys it leaves out."""
        for k in OUT_KEYS:
            ref = getattr(self, k)
            v = out.get(k) if out else None
            if v is None:
                v = ref
            elif v.device != self.device or not v.is_contiguous() or v.shape != ref.shape or v.dtype != ref.dtype:
                raise NativeError(f"output buffer {k!r} does not match the expected shape / dtype / device")
            setattr(a, k, v.data_ptr())

    def _write_consts(self, a, gvec, sgrav, scales):
        a.gravity_vec[:] = [float(x) for x in gvec]
        a.sim_gravity[:] = [float(x) for x in sgrav]
        rs = np.zeros(abi.GO1_MAX_TERMS, np.float32)
        rs[:len(scales)] = np.asarray(scales, np.float32)
        a.reward_scales[:] = [float(x) for x in rs]

    def _check_heights(self, heights, what="heights"):
        if tuple(heights.shape) != (self.n, 2, self.cfg.scan_nx, self.cfg.scan_ny) or not heights.is_contiguous() or \
                heights.dtype != torch.float32 or heights.device != self.device:
            raise NativeError(f"{what} must be a contiguous (n_envs, 2, {self.cfg.scan_nx}, {self.cfg.scan_ny}) "
                              f"float32 tensor on the env's device (go1_config.scan_nx x scan_ny)")

    def _check_optional(self, a, contact_forces, aux, obs_history, diverged_count, episode_log, log_count=None,
                        heights=None):
        """Validate the optional buffers and write their pointers (None -> NULL: the kernel skips that store).
        `episode_log` with `log_count` selects the compact log (go1_step_args.episode_log_count); `heights` receives
        the step's measured heights (go1_step_args.dbg_heights; the local planner reads them, plan.py)."""
        if heights is not None:
            self._check_heights(heights)
            a.dbg_heights = heights.data_ptr()
        a.contact_forces = self.contact_forces.data_ptr() if contact_forces else None
        if aux is not None and (not aux.is_contiguous() or aux.shape != (self.n, abi.GO1_AUX) or
                                aux.device != self.device):
            raise NativeError("aux must be a contiguous (n_envs, GO1_AUX) float32 tensor on the env's device")
        a.aux = aux.data_ptr() if aux is not None else None
        if obs_history is not None and (not obs_history.is_contiguous() or
                                        obs_history.shape != (self.n, self.cfg.num_obs)):
            raise NativeError("obs_history must be a contiguous (n_envs, num_obs) tensor")
        a.obs_history = obs_history.data_ptr() if obs_history is not None else None
        if diverged_count is not None and (diverged_count.dtype != torch.int64 or diverged_count.numel() != 1 or
                                           diverged_count.device != self.device):
            raise NativeError("diverged_count must be one int64 on the env's device")
        a.diverged_count = diverged_count.data_ptr() if diverged_count is not None else None
        a.episode_log_count, a.episode_log_cap = None, 0
        if episode_log is not None:
            w = abi.episode_log_width(self.cfg.n_terms)
            if log_count is None:
                if episode_log.shape != (self.n, w) or not episode_log.is_contiguous():
                    raise NativeError("episode_log must be a contiguous (n_envs, n_terms + 6) tensor")
            else:
                if episode_log.dim() != 2 or episode_log.shape[1] != w + 2 or not episode_log.is_contiguous() or \
                        log_count.dtype != torch.int32 or log_count.device != self.device:
                    raise NativeError("a compact episode log is a contiguous (cap, n_terms + 8) tensor + an int32 "
                                      "count")
                a.episode_log_count = log_count.data_ptr()
                a.episode_log_cap = int(episode_log.shape[0])
        a.episode_log = episode_log.data_ptr() if episode_log is not None else None

    def step(self, actions, gravity_vec, sim_gravity, reward_scales, rng_seed=0, rng_step=0, uniforms=None,
             inj=None, debug=None, events=None, episode_log=None, aux=None, out=None, obs_history=None,
             diverged_count=None, contact_forces=True):
        """One fused LeggedRobot.step on the current stream.  `debug` is an optional dict
        of preallocated tensors (torques, heights, terms, commands, reached); `out` may
        replace the default output buffers (obs, priv, rew, reset, time_out); contact_forces=False
        skips the (n, 17, 3) contact-force store (the kernel writes nothing there).

        The go1_step_args struct is kept between calls (the rollout calls this every
        few hundred microseconds); only the fields that change are rewritten."""
        a = self._args
        if a is None:
            a = self._args = self._new_args()
        self._check_actions(a, actions)
        key = (tuple(gravity_vec), tuple(sim_gravity), tuple(reward_scales))
        if key != a._consts:
            a._consts = key
            self._write_consts(a, gravity_vec, sim_gravity, reward_scales)
        a.rng_seed, a.rng_step = int(rng_seed), int(rng_step)
        if uniforms is not None and (not uniforms.is_contiguous() or uniforms.shape != (self.n, self.cfg.u_per_env)):
            raise NativeError("uniforms must be a contiguous (n_envs, u_per_env) tensor")
        a.uniforms = uniforms.data_ptr() if uniforms is not None else None
        if inj is not None:
            a.inj_dof, a.inj_root, a.inj_contact = (inj[k].data_ptr() for k in ("dof", "root", "contact"))
        else:
            a.inj_dof = a.inj_root = a.inj_contact = None
        self._check_out(a, out)
        if debug and "heights" in debug:
            self._check_heights(debug["heights"], "debug heights")
        for k, fld in (("torques", "dbg_torques"), ("heights", "dbg_heights"), ("terms", "dbg_terms"),
                       ("commands", "dbg_commands"), ("reached", "dbg_reached")):
            setattr(a, fld, debug[k].data_ptr() if debug and k in debug else None)
        self._check_optional(a, contact_forces, aux, obs_history, diverged_count, episode_log)
        a.ev_begin, a.ev_end = events if events is not None else (None, None)  # hipEvent_t pair as ints
        rc = self._lib_step(self.h, C.byref(a), self._stream())
        if rc:
            self._check(rc)

    # ------------------------------------------------------------------ per-step fast path
    def prepare(self, out, aux=None, obs_history=None, diverged_count=None, episode_log=None, log_count=None,
                contact_forces=True, heights=None):
        """A validated go1_step_args for step_prepared: the env builds one per (output-ring slot,
        episode-log half) once, so the per-step host work is a handful of field writes and the
        ctypes call (the loop is otherwise host-bound at ~60 us per step).  `episode_log` with
        `log_count` selects the compact log (go1_step_args.episode_log_count); contact_forces=False
        leaves the contact-force store out; `heights` (n_envs, 2, scan_nx, scan_ny) has the kernel store its measured
        heights (go1_step_args.dbg_heights), which it does not do otherwise."""
        a = self._new_args()
        self._check_out(a, out)
        self._check_optional(a, contact_forces, aux, obs_history, diverged_count, episode_log, log_count, heights)
        return a

    def step_prepared(self, a, actions, gravity_vec, sim_gravity, reward_scales, consts_key, rng_seed, rng_step,
                      events=None, log_tag=0):
        """go1_step with a prepare()d argument block.  `consts_key` identifies (gravity_vec,
        sim_gravity, reward_scales): they are re-copied into the block only when it changes."""
        self._check_actions(a, actions)
        if a._consts != consts_key:
            a._consts = consts_key
            self._write_consts(a, gravity_vec, sim_gravity, reward_scales)
        a.rng_seed, a.rng_step, a.episode_log_tag = rng_seed, rng_step, log_tag
        a.ev_begin, a.ev_end = events if events is not None else (None, None)
        rc = self._lib_step(self.h, C.byref(a), self._stream())
        if rc:
            self._check(rc)

    def specialize(self, enable):
        """Force the generic step kernel (False) or the README-config specialisation (True; raises
        if this config differs from it).  go1_create picks the specialisation when it applies."""
        self._check(self._lib.go1_specialize(self.h, int(bool(enable))))

    @property
    def specialized(self):
        return bool(self._lib.go1_is_specialized(self.h))

    def scan_mode(self, streamed):
        """Force the streamed height scan (True) on a 21 x 11 grid, or go back to the kernels that keep the
        scan in registers (False; raises for any other grid, which only the streamed kernel takes)."""
        self._check(self._lib.go1_scan_mode(self.h, int(bool(streamed))))

    @property
    def streamed(self):
        return bool(self._lib.go1_is_streamed(self.h))

    def sync_time_outs(self):
        """Make extras_time_outs current for the last step (the rebinding of step k is
        otherwise applied by the kernel of step k+1)."""
        self._check(self._lib.go1_sync_time_outs(self.h, self._stream()))
        return self.extras_time_outs

    def time_outs_pending(self):
        """(flag, pending, extras) device pointers of the last step's deferred extras["time_outs"]
        rebinding (None before the first step); see go1_time_outs_pending."""
        out = (C.c_int64 * 3)()
        self._check(self._lib.go1_time_outs_pending(self.h, out))
        return tuple(int(x) for x in out) if out[0] else None

    def reset_idx(self, env_ids, uniforms=None, rng_seed=0, rng_step=0):
        """go1_reset_idx for local env ids (any integer tensor; converted to int32 on the device)."""
        ids = self._ids(env_ids)
        self._check(self._lib.go1_reset_idx(self.h, ids.data_ptr(), int(ids.numel()),
                                            None if uniforms is None else uniforms.data_ptr(), int(rng_seed),
                                            int(rng_step), self._stream()))
        return ids

    def reset_envs(self, mask, uniforms=None, rng_seed=0, rng_step=0):
        m = mask.to(torch.uint8).contiguous()
        self._check(self._lib.go1_reset_envs(self.h, m.data_ptr(),
                                             None if uniforms is None else uniforms.data_ptr(), int(rng_seed),
                                             int(rng_step), self._stream()))
        return m  # keep alive until the stream passes it

    def actuator(self, x):
        x = x.contiguous()
        out = torch.empty(x.shape[0], device=x.device)
        self._check(self._lib.go1_actuator_net(self.h, x.data_ptr(), out.data_ptr(), x.shape[0], self._stream()))
        return out


def debug_buffers(n, decimation, device, grid=(abi.GO1_GRID_X, abi.GO1_GRID_Y)):
    """The optional debug outputs of go1_step; `grid` = (go1_config.scan_nx, scan_ny) of the handle."""
    return dict(torques=torch.zeros((decimation, n, 12), device=device),
                heights=torch.zeros((n, 2, int(grid[0]), int(grid[1])), device=device),
                terms=torch.zeros((n, abi.GO1_MAX_TERMS), device=device), commands=torch.zeros((n, 2), device=device),
                reached=torch.zeros(n, dtype=torch.uint8, device=device))

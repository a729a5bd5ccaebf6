"""DeviceReplay: the HBM-resident replay ring and its interchange with the reference's pickle format."""
import numpy as np

from ._rt import _torch


class _ReplayUnpickler(__import__("pickle").Unpickler):
    """pickle.Unpickler limited to the globals of replay_buffer.py's file format (replay_buffer.py:37-65)."""
    _ALLOWED = {("collections", "deque"), ("numpy", "ndarray"), ("numpy", "dtype"),
                ("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
                ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
                ("numpy.core.numeric", "_frombuffer"), ("numpy._core.numeric", "_frombuffer")}

    def find_class(self, module, name):
        if (module, name) in self._ALLOWED:
            return super().find_class(module, name)
        import pickle
        raise pickle.UnpicklingError(f"replay file refers to {module}.{name}: not part of the replay format, refused")


class DeviceReplay:
    """HBM-resident ring of (state, pi, z) tuples: the device form of replay_buffer.ReplayBuffer (deque(maxlen),
    replay_buffer.py:7-13).  Filled by Engine.emit_finished; `sample` draws uniformly without replacement
    (replay_buffer.py:15-25) and returns float32 CUDA tensors ready for the training step."""

    def __init__(self, capacity, planes, rows, cols, action_dim, device=0):
        torch = _torch()
        self.torch, self.capacity = torch, int(capacity)
        dev = torch.device("cuda", device) if isinstance(device, int) else device
        self.states = torch.zeros((capacity, planes, rows, cols), dtype=torch.float32, device=dev)
        self.pis = torch.zeros((capacity, action_dim), dtype=torch.float64, device=dev)
        self.zs = torch.zeros(capacity, dtype=torch.float32, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=dev)

    def size(self):
        return min(int(self.cursor.item()), self.capacity)

    def sample(self, batch_size, augment=None):
        """augment (OPT-IN; None: three gathers, no augmentation): "board" - every element the ring's geometry admits - or an iterable of D4
        elements (the emission's numbering, element 0 among them): each drawn row is turned by an element drawn for it from torch's generator,
        all in one azk_replay_gather launch (include/azk.h; planes and pi turned together, Connect4's pi mirrored).  For a ring that stores
        one image per position (Engine(emit_symmetry="none"))."""
        n = self.size()
        if batch_size > n:          # np.random.choice(len, batch_size, replace=False) raises the same way (replay_buffer.py:16)
            raise ValueError(f"cannot sample {batch_size} tuples without replacement from a ring holding {n}")
        idx = self.torch.randperm(n, device=self.states.device)[:batch_size]
        if augment is None:
            return self.states[idx], self.pis[idx].float(), self.zs[idx][:, None]
        draws = self.torch.randint(-(1 << 31), 1 << 31, (batch_size,), dtype=self.torch.int32, device=self.states.device)
        s, p, z = self.gather(idx, draws, self.augment_mask(augment))
        return s, p, z[:, None]

    def augment_mask(self, augment):
        """The element mask of sample's `augment`; the ring's action kind follows from action_dim: rows * cols = one action per cell, cols =
        column actions (Connect4), anything else admits the identity alone."""
        from . import board_elements
        _, _, rows, cols = self.states.shape
        A = self.pis.shape[1]
        if isinstance(augment, str):
            if augment != "board":
                raise ValueError(f"augment must be None, 'board' or an iterable of elements, not {augment!r}")
            # the elements of a Gomoku board of this shape, of Connect4's columns, or the identity alone
            els = board_elements("gomoku", (rows, cols)) if A == rows * cols else board_elements("connect4") if A == cols else (0,)
            return sum(1 << s for s in els)
        els = [int(s) for s in augment]
        if any(not 0 <= s < 32 for s in els):
            raise ValueError(f"augment: elements are 0..7, not {augment!r}")
        return sum(1 << s for s in set(els))

    def gather(self, idx, draws=None, mask=1):
        """azk_replay_gather: rows idx (int64 CUDA tensor) of the ring as (states float32, pis float32, zs float32 [n]); row b turned by
        element valid[((uint32(draws[b]) >> 16) * n_valid) >> 16] of `mask` (draws: int32 CUDA tensor, None: the identity)."""
        from . import AzkError, _p, _stream, lib
        torch = self.torch
        n = int(idx.numel())
        _, planes, rows, cols = self.states.shape
        A = self.pis.shape[1]
        idx = idx.to(torch.int64).contiguous()
        assert idx.device == self.states.device and (draws is None or (draws.dtype == torch.int32 and draws.is_contiguous() and draws.numel() == n))
        dev = self.states.device
        s = torch.empty((n, planes, rows, cols), dtype=torch.float32, device=dev)
        p = torch.empty((n, A), dtype=torch.float32, device=dev)
        z = torch.empty(n, dtype=torch.float32, device=dev)
        L = lib()
        with torch.cuda.device(dev):
            rc = L.azk_replay_gather(rows, cols, planes, A, int(mask), _p(self.states), _p(self.pis), _p(self.zs), _p(idx), _p(draws), n,
                                     _p(s), _p(p), _p(z), _stream())
        if rc != 0:
            raise AzkError(f"azk_replay_gather failed ({rc}): {L.azk_last_error(None).decode()}")
        return s, p, z

    # ---- interchange with the reference's host-side ReplayBuffer (replay_buffer.py) ------------------------------
    def add(self, state, policy_distribution, reward):
        """ReplayBuffer.add (replay_buffer.py:12): append one tuple from the host (reward: float or [float])."""
        torch = self.torch
        i = int(self.cursor.item()) % self.capacity
        self.states[i] = torch.as_tensor(np.asarray(state, np.float32))
        self.pis[i] = torch.as_tensor(np.asarray(policy_distribution, np.float64))
        self.zs[i] = float(np.asarray(reward, np.float32).reshape(-1)[0])
        self.cursor += 1

    def to_reference_deque(self):
        """The ring as the reference keeps it: deque(maxlen=capacity) of (state float32 [F,R,C], pi float64 [A], [z]) tuples,
        oldest first (train.save_data_to_buffer's element format, train.py:30-49)."""
        from collections import deque
        n, cur = self.size(), int(self.cursor.item())
        order = [(cur - n + j) % self.capacity for j in range(n)]
        s, p, z = self.states.cpu().numpy(), self.pis.cpu().numpy(), self.zs.cpu().numpy()
        return deque(((s[i].copy(), p[i].copy(), [float(z[i])]) for i in order), maxlen=self.capacity)

    def save_pickle(self, filename):
        """ReplayBuffer.save_pickle's file format (replay_buffer.py:37-54): pickle.dump of the deque."""
        import os, pickle
        folder = os.path.dirname(filename)
        if folder:
            os.makedirs(folder, exist_ok=True)
        with open(filename, "wb") as fh:
            pickle.dump(self.to_reference_deque(), fh)

    def load_pickle(self, filename):
        """Refill the ring from a file in that format (one this class or the reference's ReplayBuffer wrote).  The file is
        read by a restricted unpickler that can only build what the format holds - a deque of (ndarray, ndarray, list of
        float) - and refuses every other global, so a crafted file cannot run code."""
        with open(filename, "rb") as fh:
            items = list(_ReplayUnpickler(fh).load())[-self.capacity:]
        self.cursor.zero_()
        if items:
            torch = self.torch
            n = len(items)
            self.states[:n] = torch.as_tensor(np.stack([np.asarray(t[0], np.float32) for t in items]))
            self.pis[:n] = torch.as_tensor(np.stack([np.asarray(t[1], np.float64) for t in items]))
            self.zs[:n] = torch.as_tensor(np.array([float(np.asarray(t[2], np.float32).reshape(-1)[0]) for t in items], np.float32))
            self.cursor += n

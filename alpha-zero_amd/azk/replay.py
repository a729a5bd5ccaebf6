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

    def sample(self, batch_size):
        n = self.size()
        if batch_size > n:          # np.random.choice(len, batch_size, replace=False) raises the same way (replay_buffer.py:16)
            raise ValueError(f"cannot sample {batch_size} tuples without replacement from a ring holding {n}")
        idx = self.torch.randperm(n, device=self.states.device)[:batch_size]
        return self.states[idx], self.pis[idx].float(), self.zs[idx][:, None]

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

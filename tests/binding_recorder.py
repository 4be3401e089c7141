"""Drive heamd's device methods without a device or a built library: a recording stand-in for the loaded library notes every
C entry a method reaches and what it hands over, device tensors are CPU tensors that claim to be on the device, and every
pointer is named after the tensor it points into.  Used by test_binding_call_shapes.py and test_pir_database_file.py."""
import contextlib
import ctypes

import torch

DEGREE, MODULI, BATCH = 8, 2, 3
_zeros = torch.zeros  # (the real one, whatever recording() has put in its place)

# What the stand-in library returns, and what it writes through byref() arguments (argument index: value).
RETURNS = {"he_poly_context_degree": DEGREE, "he_poly_context_moduli_count": MODULI, "he_bfv_ciphertext_moduli_count": MODULI,
           "he_poly_serialization_byte_count": 40, "he_ciphertexts_serialization_byte_count": 90,
           "he_bfv_packed_plaintext_words": 5, "he_bfv_ciphertext_context": 0xC0}
WRITES = {
    "he_pir_database_shape": {6: 2, 7: 6, 8: 10, 9: 1, 10: 0},
    "he_pir_database_file_scan": {5: 3, 6: 2, 7: 30},
    "he_simple_pir_shape": {6: 2, 7: 3, 8: 1, 9: 4, 10: 6, 11: 1, 12: 1 << 20, 13: 1},
    "he_pnns_matrix_shape": {5: 4, 6: 2, 7: 2},
    "he_pnns_query_matrix_shape": {4: 2, 5: 1, 6: 0x1F},
}


class DeviceTensor(torch.Tensor):
    """A CPU tensor that says it is on the device."""

    @property
    def is_cuda(self):
        return True


class Stream:
    cuda_stream = 0x5EA

    def synchronize(self):
        pass


class Recorder:
    """Stands in for the ctypes library: every attribute is a function that records (name, arguments) and returns 0."""

    def __init__(self):
        self.calls, self.labels, self.keep, self.made, self.host_len = [], {Stream.cuda_stream: "stream", 0xC0: "ciphertext context"}, [], 0, 0

    # ---- tensors
    def register(self, tensor, label):
        assert tensor.numel() > 0 and tensor.data_ptr() not in self.labels, label
        self.labels[tensor.data_ptr()] = label
        self.keep.append(tensor)  # (an address names one tensor for as long as the recorder lives)
        return tensor

    def tensor(self, label, shape, dtype):
        return self.register(_zeros(shape, dtype=dtype).as_subclass(DeviceTensor), label)

    def fresh(self, tensor):
        """a tensor the method under test made itself: named new0, new1, ... in the order made"""
        self.made += 1
        if tensor.numel() == 0:
            return tensor.as_subclass(DeviceTensor)
        return self.register(tensor.as_subclass(DeviceTensor), f"new{self.made - 1}")

    # ---- the library
    def __getattr__(self, name):
        if not name.startswith("he_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append([name, [self.describe(a) for a in args]])
            for index, value in WRITES.get(name, {}).items():
                args[index]._obj.value = value
            return RETURNS.get(name, 0)

        return entry

    def pointer(self, address):
        return None if not address else self.labels.get(address, "unknown")

    def describe(self, arg):
        if arg is None or isinstance(arg, (bool, int, float, str)):
            return arg
        if isinstance(arg, ctypes.c_void_p):
            return self.pointer(arg.value)
        if isinstance(arg, ctypes.Array):
            if issubclass(arg._type_, ctypes.c_void_p):
                return [self.pointer(v) for v in arg]
            if issubclass(arg._type_, ctypes.Structure):
                return [[getattr(item, field) for field, _ in item._fields_] for item in arg]
            return list(arg)
        if isinstance(arg, ctypes._Pointer):  # a host array's pointer: the case says how many values it holds
            return [int(arg[i]) for i in range(self.host_len)]
        if type(arg).__name__ == "CArgObject":
            return "byref"
        raise TypeError(f"unexpected argument {arg!r}")

    def result(self, value):
        """dtype, shape and name of what a method returns"""
        if isinstance(value, torch.Tensor):
            return [str(value.dtype), list(value.shape), self.pointer(value.data_ptr())]
        if isinstance(value, (tuple, list)):
            return [self.result(v) for v in value]
        if isinstance(value, dict):
            return {k: self.result(v) for k, v in value.items()}
        if isinstance(value, bytes):
            return ["bytes", len(value)]
        if isinstance(value, (int, float, str, bool)) or value is None:
            return value
        return type(value).__name__


@contextlib.contextmanager
def recording(monkeypatch):
    """heamd.binding.load_library() gives a Recorder, and what the methods allocate is a DeviceTensor, inside this block."""
    import heamd

    recorder = Recorder()
    with monkeypatch.context() as patch:
        patch.setattr(heamd.binding, "load_library", lambda: recorder)
        for name in ("empty", "zeros", "empty_like", "from_numpy"):
            original = getattr(torch, name)

            def make(*args, _original=original, _name=name, **kwargs):
                kwargs.pop("device", None)
                source = args[0].as_subclass(torch.Tensor) if isinstance(args[0], torch.Tensor) else args[0]
                made = _original(source, *args[1:], **kwargs)
                return recorder.fresh(made if _name == "from_numpy" else made.fill_(0))

            patch.setattr(torch, name, make)
        patch.setattr(torch.cuda, "stream", lambda stream: contextlib.nullcontext())
        yield recorder

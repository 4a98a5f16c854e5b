"""The 9 x 29-bit-limb Montgomery core on the GPU: the fixed vectors of
test_field29.py plus 4,096 random pairs per opcode go through the device path
of the probe, and every result is bit-equal to the host path of the same
code."""
import random

import pytest
import torch

from drynx_amd import native as nt
from test_field29 import OPS, fixed_vectors, random_vectors, tensors

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("opc", OPS)
def test_device_path_is_bit_equal_to_the_host_path(opc, gpu_device):
    vecs = fixed_vectors(opc) + random_vectors(opc, 4096, random.Random(2950 + opc))
    a, b = tensors(opc, vecs)
    host = nt.field_probe(opc, a, b)
    dev = nt.field_probe(opc, a.to(gpu_device), None if b is None else b.to(gpu_device))
    assert torch.equal(dev.cpu(), host)

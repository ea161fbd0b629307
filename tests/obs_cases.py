"""Cut circuits for the marginal / expectation tests whose fragments' clbits are not contiguous."""
import random

import circuits

from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.circuit import (ClassicalRegister, QuantumCircuit,
                                                                              QuantumRegister)
from hardwareawareoptimalquantumcircuitcuttingandknitting_amd.cutting import CutSpec, cut_circuit


def _two_by_two(seed: int, n_clbits: int, measure: dict):
    rng = random.Random(seed)
    qc = QuantumCircuit(QuantumRegister(4, "q"), ClassicalRegister(n_clbits, "c"))
    circuits._rand_layer(qc, range(4), rng)
    qc.cx(0, 1)
    cut = [len(qc.data)]
    qc.cx(1, 2)
    qc.cx(3, 2)
    circuits._rand_layer(qc, range(4), rng)
    for q, c in measure.items():
        qc.measure(q, c)
    return qc, cut_circuit(qc, CutSpec([[0, 1], [2, 3]], cut))


def extra_clbit(seed: int = 21):
    """partial_measure's shape with a 5-bit register of which clbits 1 and 3 are never written:
    fragment clbits [0] and [2, 4]."""
    return _two_by_two(seed, 5, {0: 0, 2: 2, 3: 4})


def interleaved(seed: int = 22):
    """Two fully measured fragments whose clbits interleave: [0, 2] and [1, 3]."""
    return _two_by_two(seed, 4, {0: 0, 1: 2, 2: 1, 3: 3})

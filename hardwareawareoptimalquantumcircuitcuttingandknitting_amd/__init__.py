"""MI355X-native knitting hot path of HardwareAwareOptimalQuantumCircuitCuttingAndKnitting.

Public surface mirrors the reference's ``qvm`` package (``third_party/qvm/qvm``):

* :class:`VirtualCircuit`, :func:`generate_instantiations`   (``virtual_circuit.py``)
* :func:`run_virtual_circuit`, :class:`RunTimeInfo`           (``run.py``)
* :class:`QuasiDistr`                                          (``quasi_distr.py``)
* virtual gates and ``VIRTUAL_GATE_TYPES``                     (``virtual_gates.py``)

plus the circuit IR (:mod:`.circuit`), the benchmark generators and cut-spec
builder (:mod:`.generators`, :mod:`.cutting`) and the engine (:mod:`.engine`,
C ABI in ``include/qknit.h``).
"""
from .circuit import ClassicalRegister, Parameter, QuantumCircuit, QuantumRegister
from .quasi_distr import QuasiDistr
from .virtual_gates import (
    RZZ_ACCURACY,
    VIRTUAL_GATE_TYPES,
    VirtualBinaryGate,
    VirtualCPhase,
    VirtualCX,
    VirtualCY,
    VirtualCZ,
    VirtualGateEndpoint,
    VirtualMove,
    VirtualRZZ,
    WireCut,
)
from .virtual_circuit import VirtualCircuit, generate_instantiations
from .run import (RunTimeInfo, run_virtual_circuit, run_virtual_circuit_collision, run_virtual_circuit_dense,
                  run_virtual_circuit_expectation, run_virtual_circuit_fidelity, run_virtual_circuit_gradient,
                  run_virtual_circuit_marginal,
                  run_virtual_circuit_npd,
                  run_virtual_circuit_overlap, run_virtual_circuit_probabilities, run_virtual_circuit_scan,
                  run_virtual_circuit_shots, run_virtual_circuit_top_k, run_virtual_circuit_xeb)
from .parametric import ParametricKnit

__all__ = [
    "ClassicalRegister", "QuantumCircuit", "QuantumRegister", "QuasiDistr", "RZZ_ACCURACY",
    "VIRTUAL_GATE_TYPES", "VirtualBinaryGate", "VirtualCPhase", "VirtualCX", "VirtualCY",
    "VirtualCZ", "VirtualGateEndpoint", "VirtualMove", "VirtualRZZ", "WireCut", "VirtualCircuit",
    "generate_instantiations", "RunTimeInfo", "run_virtual_circuit", "run_virtual_circuit_dense",
    "run_virtual_circuit_marginal", "run_virtual_circuit_expectation", "run_virtual_circuit_gradient",
    "run_virtual_circuit_shots",
    "run_virtual_circuit_probabilities", "run_virtual_circuit_xeb", "run_virtual_circuit_collision",
    "run_virtual_circuit_overlap", "run_virtual_circuit_scan", "run_virtual_circuit_top_k",
    "run_virtual_circuit_fidelity", "run_virtual_circuit_npd", "Parameter", "ParametricKnit",
]

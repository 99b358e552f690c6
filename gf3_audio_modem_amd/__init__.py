"""gf3_audio_modem_amd -- MI355X-native OFDM receive path for the GF3 audio modem.

Layout
  csrc/      hand-written HIP kernels + the C ABI (include/gf3rx.h) -> lib/libgf3rx.so
  _lib.py    ctypes binding of that ABI (fails loudly when the library is missing)
  engine.py  Engine: torch-tensor front end of the ABI (device memory + streams only)
  ingest.py  Engine.receive_host: a stream in host memory, piece by piece, with the global-maximum rule kept exact
  OFDM.py    drop-in mirror of the reference's `receiver` class (same names/shapes)
  ldpc.py    QCLDPC: the project's quasi-cyclic LDPC codes (GPU encoder + layered min-sum decoder)
  outer.py   OuterRS: Reed-Solomon erasure code across codewords (repairs the codewords the LDPC decoder gives up on)
  loading.py adaptive bit loading: a QAM order per carrier from the measured SNR, the loaded mapper (host, NumPy)
  live.py    LiveReceiver: receive while the stream is still arriving (the self-normalised detection, piece by piece)
  crc.py     CodewordCRC: CRC-32 per codeword (catches the codewords the LDPC decoder converged on wrongly)
  dist.py    frame sharding across GPUs + the all-gather of packed bits (overlapped per chunk)
"""
from .engine import Engine, RxConfig, qpsk_table, square_qam_table  # noqa: F401
from .ldpc import QCLDPC  # noqa: F401
from .outer import OuterRS  # noqa: F401
from .crc import CodewordCRC  # noqa: F401
from .live import LiveReceiver, Segmenter, Transmission  # noqa: F401

__version__ = "0.1.0"

"""The oracle's ctypes signature table (oracle/oracle_binding.py) declares every orc_* function liboracle.so exports, and no other."""
import subprocess
from oracle import oracle_binding


def test_signature_table_declares_every_export(oracle, pkg):
    nm = subprocess.run(["nm", "-D", "--defined-only", oracle_binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {f[-1] for f in map(str.split, nm.splitlines()) if f and f[-1].startswith("orc_")}
    assert exported == set(oracle_binding.signatures(pkg._abi, oracle.AO))

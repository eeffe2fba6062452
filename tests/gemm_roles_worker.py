"""child process of tests/test_gpu_gemm_roles.py: the hashes of the batch-9 congruence cases' and the nz = 16 Gram case's outputs,
printed as JSON, under whatever HDM_PERSIST the parent set (the library reads it once per process)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import test_gpu_gemm_roles as roles  # noqa: E402

print("GEMM_ROLES_WORKER_JSON " + json.dumps(roles.launch_form_hashes()))

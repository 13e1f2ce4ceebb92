"""Child processes of the GPU tests, one at a time, each under its own time limit -- and none at all after one of them has
faulted: a child that times out, dies on a signal, exits with 124 / 134 / 137 / 139 or reports a HIP illegal memory access sets
the runner's stop flag, and every later call fails at once WITHOUT starting a process (a card that has faulted is left alone
until the cause is known)."""
import subprocess

FAULT_CODES = (124, 134, 137, 139)  # a time limit, SIGABRT, SIGKILL, SIGSEGV as a shell reports them
FAULT_TEXT = "an illegal memory access was encountered"
TIMEOUT = 120  # seconds: the limit the C++ consumer tests have always used


class ChildFault(AssertionError):
    pass


class ChildRunner:
    def __init__(self):
        self.stopped = None  # why no further child is started
        self.started = 0

    def run(self, argv, env=None, timeout=TIMEOUT):
        """subprocess.run(argv) with the output captured; raises ChildFault instead where the stop flag is set, and sets it
        where this child faults."""
        if self.stopped:
            raise ChildFault(f"not started: an earlier child process faulted ({self.stopped})")
        self.started += 1
        try:
            out = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            self.stopped = f"{argv[:3]} ran into its {timeout} s limit"
            raise ChildFault(self.stopped)
        if out.returncode < 0 or out.returncode in FAULT_CODES or FAULT_TEXT in out.stdout or FAULT_TEXT in out.stderr:
            self.stopped = f"{argv[:3]} ended with {out.returncode}: {(out.stdout + out.stderr)[-400:]}"
            raise ChildFault(self.stopped)
        return out


RUNNER = ChildRunner()  # the one every GPU test module shares

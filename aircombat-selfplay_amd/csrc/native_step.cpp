// VecEnv.step in one native call (vec_env.py: HipVecEnv.step / HipShareVecEnv.step): the host bookkeeping of a step -- which result set,
// where the caller's actions are, the tuple and the LazyInfos handed back -- without the interpreter, and with the object construction
// placed between ac_step_host_actions_begin and ac_step_host_actions_wait, where the kernel is already running. A CPython extension on
// the plain C API; it links to nothing of HIP: the two entry points and the handle arrive as raw addresses from the loaded capi.Lib.
//
// Whatever this path does not take -- a ring that has to grow or stage, actions that need converting -- it answers with None and changes
// nothing, and the Python code runs as before.
#define PY_SSIZE_T_CLEAN
#include <Python.h>
#include <structmember.h>

#include <cstddef>
#include <cstdint>

#include "native_step_pick.hpp"

namespace {

using begin_fn = int (*)(void*, int32_t, const float*, size_t);
using wait_fn = int (*)(void*);

struct SetRec {
  PyObject* out;                                   // the set's tuple of arrays (st["out"]): the only holder of the arrays besides `result`
  PyObject* result;                                // copy=False: what step() returns for the set, built once; else null
  Py_ssize_t baseline[native_step::MAX_ARRAYS];    // the arrays' reference counts when add_set was called: nobody outside holds them
};

struct Stepper {
  PyObject_HEAD
  begin_fn begin;
  wait_fn wait;
  void* handle;
  size_t n_floats;
  int copy, share, n_arrays, n_sets;
  SetRec sets[native_step::MAX_SETS];
  PyObject* lazy_infos;   // the LazyInfos class
  PyObject* check;        // lib.check: raises the library's error as the ctypes path does
};

PyObject* g_cur_name = nullptr;       // "_cur", interned
PyObject* g_failed_name = nullptr;    // "ac_step_host_actions"
PyObject* g_minus_one = nullptr;

void* address_arg(PyObject* o) { return PyLong_AsVoidPtr(o); }

int stepper_init(PyObject* self_, PyObject* args, PyObject* kwds) {
  Stepper* s = (Stepper*)self_;
  static const char* names[] = {"begin", "wait", "handle", "n_floats", "copy", "share", "lazy_infos", "check", nullptr};
  PyObject *b, *w, *h, *lazy, *check;
  Py_ssize_t n;
  int copy, share;
  if (!PyArg_ParseTupleAndKeywords(args, kwds, "OOOnppOO", (char**)names, &b, &w, &h, &n, &copy, &share, &lazy, &check)) return -1;
  void* bp = address_arg(b);
  void* wp = address_arg(w);
  void* hp = address_arg(h);
  if (PyErr_Occurred()) return -1;
  if (!bp || !wp || !hp || n <= 0 || !PyCallable_Check(lazy) || !PyCallable_Check(check)) {
    PyErr_SetString(PyExc_ValueError, "Stepper: null address, empty batch or a non-callable");
    return -1;
  }
  s->begin = (begin_fn)bp;
  s->wait = (wait_fn)wp;
  s->handle = hp;
  s->n_floats = (size_t)n;
  s->copy = copy;
  s->share = share;
  s->n_arrays = share ? 5 : 4;
  Py_INCREF(lazy);
  Py_XSETREF(s->lazy_infos, lazy);
  Py_INCREF(check);
  Py_XSETREF(s->check, check);
  return 0;
}

void stepper_clear_sets(Stepper* s) {
  const int n = s->n_sets;
  s->n_sets = 0;
  for (int k = 0; k < n; ++k) {
    Py_CLEAR(s->sets[k].out);
    Py_CLEAR(s->sets[k].result);
  }
}

void stepper_dealloc(PyObject* self_) {
  Stepper* s = (Stepper*)self_;
  stepper_clear_sets(s);
  Py_CLEAR(s->lazy_infos);
  Py_CLEAR(s->check);
  Py_TYPE(self_)->tp_free(self_);
}

// add_set(out, result): set number n_sets of the ring. Called when the set is created, after everything inside the VecEnv that refers to
// its arrays exists: the counts seen here are the baseline.
PyObject* stepper_add_set(PyObject* self_, PyObject* const* args, Py_ssize_t nargs) {
  Stepper* s = (Stepper*)self_;
  if (nargs != 2 || !PyTuple_CheckExact(args[0]) || PyTuple_GET_SIZE(args[0]) != s->n_arrays) {
    PyErr_SetString(PyExc_TypeError, "add_set(out, result): out is the set's tuple of arrays");
    return nullptr;
  }
  if (s->n_sets >= native_step::MAX_SETS) {
    PyErr_SetString(PyExc_ValueError, "add_set: the ring is full");
    return nullptr;
  }
  if (!s->copy && !PyTuple_CheckExact(args[1])) {
    PyErr_SetString(PyExc_TypeError, "add_set: with copy=False result is the tuple step() returns for the set");
    return nullptr;
  }
  SetRec& r = s->sets[s->n_sets];
  Py_INCREF(args[0]);
  r.out = args[0];
  r.result = nullptr;
  if (!s->copy) {
    Py_INCREF(args[1]);
    r.result = args[1];
  }
  for (int i = 0; i < s->n_arrays; ++i) r.baseline[i] = Py_REFCNT(PyTuple_GET_ITEM(r.out, i));
  s->n_sets += 1;
  Py_RETURN_NONE;
}

bool set_held(const Stepper* s, int k) {
  const SetRec& r = s->sets[k];
  Py_ssize_t now[native_step::MAX_ARRAYS];
  for (int i = 0; i < s->n_arrays; ++i) now[i] = Py_REFCNT(PyTuple_GET_ITEM(r.out, i));
  return native_step::held(now, r.baseline, s->n_arrays);
}

PyObject* stepper_held(PyObject* self_, PyObject* arg) {
  Stepper* s = (Stepper*)self_;
  const long k = PyLong_AsLong(arg);
  if (k == -1 && PyErr_Occurred()) return nullptr;
  if (k < 0 || k >= s->n_sets) {
    PyErr_SetString(PyExc_IndexError, "held: no such set");
    return nullptr;
  }
  return PyBool_FromLong(set_held(s, (int)k));
}

PyObject* stepper_clear(PyObject* self_, PyObject*) {
  stepper_clear_sets((Stepper*)self_);
  Py_RETURN_NONE;
}

// What step() hands back for set k. copy=False: the tuple built once. Default: the set's own arrays in a new tuple with a new LazyInfos
// over the info words (HipVecEnv._owned / HipShareVecEnv._owned).
PyObject* build_result(Stepper* s, int k) {
  SetRec& r = s->sets[k];
  if (!s->copy) {
    Py_INCREF(r.result);
    return r.result;
  }
  PyObject* infos = PyObject_CallFunctionObjArgs(s->lazy_infos, PyTuple_GET_ITEM(r.out, 3), nullptr);
  if (!infos) return nullptr;
  PyObject* t = PyTuple_New(s->share ? 5 : 4);
  if (!t) {
    Py_DECREF(infos);
    return nullptr;
  }
  static const int plain[3] = {0, 1, 2}, shared[4] = {0, 4, 1, 2};   // (obs, [share_obs,] rewards, dones, infos)
  const int* order = s->share ? shared : plain;
  const int n = s->share ? 4 : 3;
  for (int i = 0; i < n; ++i) {
    PyObject* a = PyTuple_GET_ITEM(r.out, order[i]);
    Py_INCREF(a);
    PyTuple_SET_ITEM(t, i, a);
  }
  PyTuple_SET_ITEM(t, n, infos);
  return t;
}

PyObject* raise_library_error(Stepper* s) {
  PyObject* r = PyObject_CallFunctionObjArgs(s->check, g_minus_one, g_failed_name, nullptr);
  if (r) {   // (check raises for a non-zero code; should it ever not, the failure still surfaces)
    Py_DECREF(r);
    PyErr_SetString(PyExc_RuntimeError, "ac_step_host_actions failed");
  }
  return nullptr;
}

// step(env, actions) -> the step's result, or None where the Python path has to run (nothing has been changed then).
PyObject* stepper_step(PyObject* self_, PyObject* const* args, Py_ssize_t nargs) {
  Stepper* s = (Stepper*)self_;
  if (nargs != 2) {
    PyErr_SetString(PyExc_TypeError, "step(env, actions)");
    return nullptr;
  }
  PyObject* env = args[0];
  PyObject* actions = args[1];
  // 1. the set of this step
  PyObject* cur_obj = PyObject_GetAttr(env, g_cur_name);
  if (!cur_obj) return nullptr;
  const long cur_l = PyLong_AsLong(cur_obj);
  Py_DECREF(cur_obj);
  if (cur_l == -1 && PyErr_Occurred()) return nullptr;
  const int cur = (cur_l < 0 || cur_l >= native_step::MAX_SETS) ? -1 : (int)cur_l;
  int k;
  if (!s->copy) k = s->n_sets >= 2 ? native_step::pick_alternate(cur) : native_step::FALLBACK;
  else k = native_step::pick_ring(cur, s->n_sets, [s](int i) { return set_held(s, i); });
  if (k == native_step::FALLBACK) Py_RETURN_NONE;
  // 2. the caller's batch, where it is
  if (!PyObject_CheckBuffer(actions)) Py_RETURN_NONE;
  Py_buffer view;
  if (PyObject_GetBuffer(actions, &view, PyBUF_C_CONTIGUOUS | PyBUF_FORMAT) != 0) {   // (a strided slice; read-only is fine)
    PyErr_Clear();
    Py_RETURN_NONE;
  }
  if (!native_step::fast_actions(view.format, view.itemsize, view.len, s->n_floats)) {
    PyBuffer_Release(&view);
    Py_RETURN_NONE;
  }
  // header word, doorbell, copy under the launch
  const int rc_begin = s->begin(s->handle, (int32_t)k, (const float*)view.buf, s->n_floats);
  PyBuffer_Release(&view);   // (the library has copied the batch)
  // from here on the kernel runs: everything up to the wait is off the critical path
  PyObject* idx = PyLong_FromLong(k);
  const int set_rc = idx ? PyObject_SetAttr(env, g_cur_name, idx) : -1;
  Py_XDECREF(idx);
  if (rc_begin != 0) {
    PyErr_Clear();
    return raise_library_error(s);
  }
  // 3. what the caller gets
  PyObject* result = set_rc == 0 ? build_result(s, k) : nullptr;
  PyObject *et = nullptr, *ev = nullptr, *tb = nullptr;
  if (!result) PyErr_Fetch(&et, &ev, &tb);   // the step is in flight all the same: wait for it, then report
  // 4. the wait, and only the wait, without the GIL: MultiDeviceVecEnv steps its handles from threads
  int rc;
  Py_BEGIN_ALLOW_THREADS
  rc = s->wait(s->handle);
  Py_END_ALLOW_THREADS
  if (!result) {
    PyErr_Restore(et, ev, tb);
    return nullptr;
  }
  // 5. a HIP failure, a non-finite aircraft state ("JSBSim failed."), rows that never arrived
  if (rc != 0) {
    Py_DECREF(result);
    return raise_library_error(s);
  }
  return result;
}

PyMethodDef stepper_methods[] = {
    {"step", (PyCFunction)(void (*)(void))stepper_step, METH_FASTCALL, "step(env, actions) -> result tuple, or None: take the Python path"},
    {"add_set", (PyCFunction)(void (*)(void))stepper_add_set, METH_FASTCALL, "add_set(out, result): the next set of the ring; records the baseline counts"},
    {"held", stepper_held, METH_O, "held(k): does anybody outside hold an array of set k"},
    {"clear", stepper_clear, METH_NOARGS, "drop every set (close())"},
    {nullptr, nullptr, 0, nullptr}};

PyMemberDef stepper_members[] = {{"n_sets", T_INT, offsetof(Stepper, n_sets), READONLY, "sets in the ring"}, {nullptr, 0, 0, 0, nullptr}};

PyTypeObject StepperType = {PyVarObject_HEAD_INIT(nullptr, 0)};

PyModuleDef moduledef = {PyModuleDef_HEAD_INIT, "_native_step", "VecEnv.step without the interpreter (csrc/native_step.cpp)", -1, nullptr, nullptr, nullptr, nullptr, nullptr};

}  // namespace

PyMODINIT_FUNC PyInit__native_step(void) {
  StepperType.tp_name = "_native_step.Stepper";
  StepperType.tp_basicsize = sizeof(Stepper);
  StepperType.tp_flags = Py_TPFLAGS_DEFAULT;
  StepperType.tp_doc = "Stepper(begin, wait, handle, n_floats, copy, share, lazy_infos, check)";
  StepperType.tp_new = PyType_GenericNew;
  StepperType.tp_init = stepper_init;
  StepperType.tp_dealloc = stepper_dealloc;
  StepperType.tp_methods = stepper_methods;
  StepperType.tp_members = stepper_members;
  if (PyType_Ready(&StepperType) < 0) return nullptr;
  g_cur_name = PyUnicode_InternFromString("_cur");
  g_failed_name = PyUnicode_InternFromString("ac_step_host_actions");
  g_minus_one = PyLong_FromLong(-1);
  if (!g_cur_name || !g_failed_name || !g_minus_one) return nullptr;
  PyObject* m = PyModule_Create(&moduledef);
  if (!m) return nullptr;
  Py_INCREF(&StepperType);
  if (PyModule_AddObject(m, "Stepper", (PyObject*)&StepperType) < 0) {
    Py_DECREF(&StepperType);
    Py_DECREF(m);
    return nullptr;
  }
  return m;
}

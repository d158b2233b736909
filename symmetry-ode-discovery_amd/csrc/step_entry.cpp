// _symode_step: the host side of one step on the reduced form (symode_quad_step) as ONE native call.
//
// A host-only CPython extension.  It holds no device code and does not link libsymode_hip.so: a Plan is given the address of
// symode_quad_step as an integer, taken from the handle the engine already holds, so the process keeps one copy of the
// library and the library's SYMODE_* switches stay its own.  What engine.ReducedStep and BatchedClosure.evaluate did per
// call in Python -- the twelve-component key, the row checks, one packed allocation, the current stream, the sixteen-argument
// call, three views -- is done here on the tensors themselves; the call imports nothing and calls no Python-level function.
//
// A call answers one of
//   (loss, g_beta, g_const or None)   the step was launched
//   None                              the library refused (SYMODE_E_UNSUPPORTED, a switch): take the one-launch kernel
//   STALE                             the key moved: build the form again
//   SLOW                              an operand has to be made dense or is of the wrong kind: engine.ReducedStep copies or raises
//   another int                       the library's error code (a HIP error if positive), for HipEngine._check
#define PY_SSIZE_T_CLEAN
#include <Python.h>
#include <structmember.h>

#include <cstddef>
#include <cstdint>
#include <new>

#include <ATen/core/LegacyTypeDispatch.h>
#include <ATen/core/Tensor.h>
#include <ATen/ops/as_strided.h>
#include <ATen/ops/empty.h>
#include <c10/core/Device.h>
#include <c10/hip/HIPStream.h>
#include <torch/csrc/autograd/python_variable.h>

namespace {

// symode_quad_step of include/symode.h
using quad_step_fn = int (*)(const double*, long, int, int, int, unsigned long long, const float*, long, const float*, long, float*,
                             float*, float*, void*, size_t, void*);

constexpr long STALE = -1001, SLOW = -1002;    // clear of the SYMODE_E_* codes of include/symode.h
constexpr int E_UNSUPPORTED = -1;                    // SYMODE_E_UNSUPPORTED
constexpr int N_KEY_TENSORS = 5;                     // x, dx, gx, jgx, Q

struct TensorKey {
    int64_t version;
    const void* ptr;
};

struct Key {
    TensorKey t[N_KEY_TENSORS];
    double weight;
    bool live_none;
    unsigned long long live;
};

struct Plan {
    PyObject_HEAD
    vectorcallfunc vectorcall;
    quad_step_fn fn;
    at::Tensor B, ws;                                // kept alive with the pointers below
    at::Tensor alias_buf;
    PyObject* alias_views;                           // the tuple an ``alias`` call returns, made at the first one
    PyObject* slow;                                  // whatever the caller wants to find here: the engine keeps its ReducedStep
    long S;
    int r, dc, order;
    unsigned long long live;
    size_t ws_bytes;
    int64_t n_out;
    Key key;
    bool constructed;
};

bool tensor_arg(PyObject* o, const char* name) {
    if (THPVariable_Check(o)) return true;
    PyErr_Format(PyExc_TypeError, "%s must be a torch.Tensor, not %s", name, Py_TYPE(o)->tp_name);
    return false;
}

// (x, dx, (gx, jgx, weight), Q, live) -> the twelve components of BatchedClosure._reduced_key
bool read_key(PyObject* x, PyObject* dx, PyObject* sym, PyObject* Q, PyObject* live, Key& k) {
    if (!PyTuple_CheckExact(sym) || PyTuple_GET_SIZE(sym) != 3) {
        PyErr_SetString(PyExc_TypeError, "sym must be the tuple (gx, jgx, weight)");
        return false;
    }
    PyObject* parts[N_KEY_TENSORS] = {x, dx, PyTuple_GET_ITEM(sym, 0), PyTuple_GET_ITEM(sym, 1), Q};
    static const char* const names[N_KEY_TENSORS] = {"x", "dx", "gx", "jgx", "Q"};
    for (int i = 0; i < N_KEY_TENSORS; ++i) {
        if (!tensor_arg(parts[i], names[i])) return false;
        const at::Tensor& t = THPVariable_Unpack(parts[i]);
        k.t[i].version = t._version();
        k.t[i].ptr = t.data_ptr();
    }
    PyObject* w = PyTuple_GET_ITEM(sym, 2);
    k.weight = PyFloat_CheckExact(w) ? PyFloat_AS_DOUBLE(w) : PyFloat_AsDouble(w);
    if (k.weight == -1.0 && PyErr_Occurred()) return false;
    k.live_none = live == Py_None;
    k.live = 0;
    if (!k.live_none) {
        if (!PyLong_Check(live)) {
            PyErr_SetString(PyExc_TypeError, "live must be an int or None");
            return false;
        }
        k.live = PyLong_AsUnsignedLongLongMask(live);
        if (k.live == (unsigned long long)-1 && PyErr_Occurred()) return false;
    }
    return true;
}

bool same_key(const Key& a, const Key& b) {
    for (int i = 0; i < N_KEY_TENSORS; ++i)
        if (a.t[i].version != b.t[i].version || a.t[i].ptr != b.t[i].ptr) return false;
    return a.weight == b.weight && a.live_none == b.live_none && a.live == b.live;
}

// ReducedStep._rows without its slow half: the row stride of an (S, w[, 1]) fp32 operand that can be read where it lies, or -1
long row_stride(const at::Tensor& t, const c10::Device& dev, long S, long w) {
    if (t.scalar_type() != at::kFloat || t.device() != dev || t.dim() < 2) return -1;
    const auto sizes = t.sizes();
    const auto strides = t.strides();
    if (sizes[0] != S || sizes[1] != w || t.numel() != S * w || strides[1] != 1 || !(strides[0] >= w || S == 1)) return -1;
    return S > 1 ? (long)strides[0] : w;
}

// (loss (S,), g_beta (S, r), g_const (S, d_c, 1) or None) on the packed buffer [loss | g_beta | g_const]
PyObject* make_views(const Plan* p, const at::Tensor& buf) {
    const int64_t S = p->S, r = p->r, dc = p->dc;
    PyObject* out = PyTuple_New(3);
    if (!out) return nullptr;
    PyTuple_SET_ITEM(out, 0, THPVariable_Wrap(at::as_strided(buf, {S}, {1}, 0)));
    PyTuple_SET_ITEM(out, 1, THPVariable_Wrap(at::as_strided(buf, {S, r}, {r, 1}, S)));
    if (dc) {
        PyTuple_SET_ITEM(out, 2, THPVariable_Wrap(at::as_strided(buf, {S, dc, 1}, {dc, 1, 1}, S * (1 + r))));
    } else {
        Py_INCREF(Py_None);
        PyTuple_SET_ITEM(out, 2, Py_None);
    }
    for (int i = 0; i < 3; ++i)
        if (!PyTuple_GET_ITEM(out, i)) {
            Py_DECREF(out);
            return nullptr;
        }
    return out;
}

// plan((anything, beta, const, alias, x, dx, sym, Q, live)): the tuple engine.loss_grad_reversed(reduced=...) hands on
PyObject* plan_step(Plan* p, PyObject* args) {
    if (!PyTuple_CheckExact(args) || PyTuple_GET_SIZE(args) != 9) {
        PyErr_SetString(PyExc_TypeError, "the step takes the tuple (plan, beta, const, alias, x, dx, sym, Q, live)");
        return nullptr;
    }
    PyObject* beta_o = PyTuple_GET_ITEM(args, 1);
    PyObject* const_o = PyTuple_GET_ITEM(args, 2);
    const int alias = PyObject_IsTrue(PyTuple_GET_ITEM(args, 3));
    if (alias < 0) return nullptr;
    Key now;
    if (!read_key(PyTuple_GET_ITEM(args, 4), PyTuple_GET_ITEM(args, 5), PyTuple_GET_ITEM(args, 6), PyTuple_GET_ITEM(args, 7),
                  PyTuple_GET_ITEM(args, 8), now))
        return nullptr;
    if (!tensor_arg(beta_o, "beta") || (p->dc && !tensor_arg(const_o, "const"))) return nullptr;
    if (!same_key(now, p->key)) return PyLong_FromLong(STALE);

    const c10::Device dev = p->B.device();
    const at::Tensor& beta = THPVariable_Unpack(beta_o);
    const long ldb = row_stride(beta, dev, p->S, p->r);
    if (ldb < 0) return PyLong_FromLong(SLOW);
    const float* cptr = nullptr;
    long ldc = 0;
    if (p->dc) {
        const at::Tensor& c = THPVariable_Unpack(const_o);
        ldc = row_stride(c, dev, p->S, p->dc);
        if (ldc < 0) return PyLong_FromLong(SLOW);
        cptr = (const float*)c.data_ptr();
    }

    // below autograd and view tracking: the outputs are plain tensors on one storage, without history
    at::AutoDispatchBelowADInplaceOrView below;
    at::Tensor fresh;
    if (alias) {
        if (!p->alias_views) {
            p->alias_buf = at::empty({p->n_out}, p->B.options().dtype(at::kFloat));
            p->alias_views = make_views(p, p->alias_buf);
            if (!p->alias_views) return nullptr;
        }
    } else {
        fresh = at::empty({p->n_out}, p->B.options().dtype(at::kFloat));
    }
    const at::Tensor& buf = alias ? p->alias_buf : fresh;
    float* base = (float*)buf.data_ptr();
    void* stream = dev.is_cuda() ? (void*)c10::hip::getCurrentHIPStream(dev.index()).stream() : nullptr;
    const int rc = p->fn((const double*)p->B.data_ptr(), p->S, p->r + p->dc, p->dc, p->order, p->live, (const float*)beta.data_ptr(),
                         ldb, cptr, ldc, base, base + p->S, p->dc ? base + p->S * (1 + p->r) : nullptr, p->ws.data_ptr(),
                         p->ws_bytes, stream);
    if (rc == E_UNSUPPORTED) Py_RETURN_NONE;
    if (rc != 0) return PyLong_FromLong(rc);
    if (alias) {
        Py_INCREF(p->alias_views);
        return p->alias_views;
    }
    return make_views(p, fresh);
}

PyObject* plan_vectorcall(PyObject* self, PyObject* const* args, size_t nargsf, PyObject* kwnames) {
    if (PyVectorcall_NARGS(nargsf) != 1 || (kwnames && PyTuple_GET_SIZE(kwnames))) {
        PyErr_SetString(PyExc_TypeError, "the step takes one argument, the tuple (plan, beta, const, alias, x, dx, sym, Q, live)");
        return nullptr;
    }
    try {
        return plan_step((Plan*)self, args[0]);
    } catch (const std::exception& e) {
        PyErr_SetString(PyExc_RuntimeError, e.what());
        return nullptr;
    }
}

// Plan(fn_address, B, ws, r, dc, order, live, key, slow=None); key = (x, dx, sym, Q, live) as a call passes them
int plan_init(PyObject* self, PyObject* args, PyObject* kwargs) {
    Plan* p = (Plan*)self;
    static const char* kwlist[] = {"fn_address", "B", "ws", "r", "dc", "order", "live", "key", "slow", nullptr};
    unsigned long long addr = 0, live = 0;
    PyObject *B_o, *ws_o, *key_o, *slow = Py_None;
    int r, dc, order;
    if (!PyArg_ParseTupleAndKeywords(args, kwargs, "KOOiiiKO|O", (char**)kwlist, &addr, &B_o, &ws_o, &r, &dc, &order, &live, &key_o, &slow))
        return -1;
    if (p->constructed) {
        PyErr_SetString(PyExc_RuntimeError, "a Plan is initialised once");
        return -1;
    }
    if (!addr) {
        PyErr_SetString(PyExc_ValueError, "fn_address is null");
        return -1;
    }
    if (!tensor_arg(B_o, "B") || !tensor_arg(ws_o, "ws")) return -1;
    if (!PyTuple_CheckExact(key_o) || PyTuple_GET_SIZE(key_o) != 5) {
        PyErr_SetString(PyExc_TypeError, "key must be the tuple (x, dx, sym, Q, live)");
        return -1;
    }
    try {
        const at::Tensor& B = THPVariable_Unpack(B_o);
        const at::Tensor& ws = THPVariable_Unpack(ws_o);
        const long K = (long)r + dc;
        if (B.scalar_type() != at::kDouble || B.dim() != 3 || B.size(0) < 1 || B.size(1) != K + 1 || B.size(2) != K + 1 || r < 1 ||
            dc < 0 || K + 1 > 16 || !B.is_contiguous()) {
            PyErr_SetString(PyExc_ValueError, "B must hold (S, K+1, K+1) float64, contiguous, for K = r + dc <= 15");
            return -1;
        }
        if (ws.scalar_type() != at::kDouble || ws.device() != B.device() || !ws.is_contiguous()) {
            PyErr_SetString(PyExc_ValueError, "ws must be a contiguous float64 workspace on B's device");
            return -1;
        }
        Key key;
        if (!read_key(PyTuple_GET_ITEM(key_o, 0), PyTuple_GET_ITEM(key_o, 1), PyTuple_GET_ITEM(key_o, 2), PyTuple_GET_ITEM(key_o, 3),
                      PyTuple_GET_ITEM(key_o, 4), key))
            return -1;
        p->fn = (quad_step_fn)(uintptr_t)addr;
        p->B = B;
        p->ws = ws;
        p->S = (long)B.size(0);
        p->r = r;
        p->dc = dc;
        p->order = order;
        p->live = live;
        p->ws_bytes = (size_t)ws.numel() * 8;
        p->n_out = (int64_t)p->S * (1 + r + dc);
        p->key = key;
        Py_INCREF(slow);
        Py_XSETREF(p->slow, slow);
        p->constructed = true;
        return 0;
    } catch (const std::exception& e) {
        PyErr_SetString(PyExc_RuntimeError, e.what());
        return -1;
    }
}

PyObject* plan_new(PyTypeObject* type, PyObject*, PyObject*) {
    Plan* p = (Plan*)type->tp_alloc(type, 0);
    if (!p) return nullptr;
    new (&p->B) at::Tensor();
    new (&p->ws) at::Tensor();
    new (&p->alias_buf) at::Tensor();
    p->vectorcall = plan_vectorcall;
    p->fn = nullptr;
    p->alias_views = nullptr;
    Py_INCREF(Py_None);
    p->slow = Py_None;
    p->constructed = false;
    return (PyObject*)p;
}

int plan_traverse(PyObject* self, visitproc visit, void* arg) {
    Plan* p = (Plan*)self;
    Py_VISIT(p->alias_views);
    Py_VISIT(p->slow);
    return 0;
}

int plan_clear(PyObject* self) {
    Plan* p = (Plan*)self;
    Py_CLEAR(p->alias_views);
    Py_CLEAR(p->slow);
    return 0;
}

void plan_dealloc(PyObject* self) {
    Plan* p = (Plan*)self;
    PyObject_GC_UnTrack(self);
    plan_clear(self);
    p->alias_buf.~Tensor();
    p->ws.~Tensor();
    p->B.~Tensor();
    Py_TYPE(self)->tp_free(self);
}

// (buffer, (loss, g_beta, g_const or None)) of ``alias`` calls, made here if no such call came yet: the slow path writes there too
PyObject* plan_alias_buffers(PyObject* self, PyObject*) {
    Plan* p = (Plan*)self;
    if (!p->constructed) {
        PyErr_SetString(PyExc_RuntimeError, "the Plan is not initialised");
        return nullptr;
    }
    try {
        at::AutoDispatchBelowADInplaceOrView below;
        if (!p->alias_views) {
            p->alias_buf = at::empty({p->n_out}, p->B.options().dtype(at::kFloat));
            p->alias_views = make_views(p, p->alias_buf);
            if (!p->alias_views) return nullptr;
        }
        PyObject* buf = THPVariable_Wrap(p->alias_buf);
        if (!buf) return nullptr;
        PyObject* out = PyTuple_Pack(2, buf, p->alias_views);
        Py_DECREF(buf);
        return out;
    } catch (const std::exception& e) {
        PyErr_SetString(PyExc_RuntimeError, e.what());
        return nullptr;
    }
}

PyObject* plan_get_B(PyObject* self, void*) { return THPVariable_Wrap(((Plan*)self)->B); }
PyObject* plan_get_ws(PyObject* self, void*) { return THPVariable_Wrap(((Plan*)self)->ws); }
PyObject* plan_get_live(PyObject* self, void*) { return PyLong_FromUnsignedLongLong(((Plan*)self)->live); }
PyObject* plan_get_ws_bytes(PyObject* self, void*) { return PyLong_FromSize_t(((Plan*)self)->ws_bytes); }

PyMethodDef plan_methods[] = {
    {"alias_buffers", plan_alias_buffers, METH_NOARGS, "(buffer, (loss, g_beta, g_const or None)) that ``alias`` calls write and return"},
    {nullptr, nullptr, 0, nullptr}};

PyMemberDef plan_members[] = {
    {"S", T_LONG, offsetof(Plan, S), READONLY, "problems"},
    {"r", T_INT, offsetof(Plan, r), READONLY, "columns of Q"},
    {"dc", T_INT, offsetof(Plan, dc), READONLY, "constants per problem"},
    {"order", T_INT, offsetof(Plan, order), READONLY, "polynomial order of the closure B was reduced from"},
    {"slow", T_OBJECT, offsetof(Plan, slow), READONLY, "the object given as ``slow``"},
    {nullptr, 0, 0, 0, nullptr}};

PyGetSetDef plan_getset[] = {
    {"B", plan_get_B, nullptr, "the reduced form", nullptr},
    {"ws", plan_get_ws, nullptr, "the workspace", nullptr},
    {"live", plan_get_live, nullptr, "the column set handed to the library", nullptr},
    {"ws_bytes", plan_get_ws_bytes, nullptr, "bytes of the workspace", nullptr},
    {nullptr, nullptr, nullptr, nullptr, nullptr}};

PyTypeObject PlanType = {PyVarObject_HEAD_INIT(nullptr, 0)};

PyModuleDef module_def = {PyModuleDef_HEAD_INIT, "_symode_step",
                          "The step on the reduced form as one native call (csrc/step_entry.cpp).", -1, nullptr};

}  // namespace

PyMODINIT_FUNC PyInit__symode_step(void) {
    PlanType.tp_name = "_symode_step.Plan";
    PlanType.tp_doc = "A prepared symode_quad_step launch on one reduced form B; call it with the tuple of engine.loss_grad_reversed(reduced=).";
    PlanType.tp_basicsize = sizeof(Plan);
    PlanType.tp_flags = Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC | Py_TPFLAGS_HAVE_VECTORCALL;
    PlanType.tp_new = plan_new;
    PlanType.tp_init = plan_init;
    PlanType.tp_dealloc = plan_dealloc;
    PlanType.tp_traverse = plan_traverse;
    PlanType.tp_clear = plan_clear;
    PlanType.tp_call = PyVectorcall_Call;
    PlanType.tp_vectorcall_offset = offsetof(Plan, vectorcall);
    PlanType.tp_methods = plan_methods;
    PlanType.tp_members = plan_members;
    PlanType.tp_getset = plan_getset;
    if (PyType_Ready(&PlanType) < 0) return nullptr;
    PyObject* m = PyModule_Create(&module_def);
    if (!m) return nullptr;
    Py_INCREF(&PlanType);
    if (PyModule_AddObject(m, "Plan", (PyObject*)&PlanType) < 0 || PyModule_AddIntConstant(m, "STALE", STALE) < 0 ||
        PyModule_AddIntConstant(m, "SLOW", SLOW) < 0) {
        Py_DECREF(m);
        return nullptr;
    }
    return m;
}

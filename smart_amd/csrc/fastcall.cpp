// smart_amd._fastcall: the calls of engine.py that sit in a caller's loop, bound without ctypes.
//
// Plan.launch through ctypes costs about a microsecond (two foreign calls, six converted arguments, the GIL released
// and taken again), several times what smartgpu_plan_launch itself takes to queue a launch.  This module gives
// engine.Text and engine.Plan a base type each:
//   TextBase  keeps the handle (`_h`: an int, or None after free()) and the text's length, read ONCE through
//             smartgpu_text_length when the handle is set (a text is never resized);
//   PlanBase  keeps the handle and implements launch(text, slot=0, timed=False, off=0, n=None).
// The library is reached through function pointers that engine.py hands over as integers (_bind), taken from the
// library that made the object: this module links neither libsmartgpu.so nor libpython, so SMARTGPU_LIB,
// use_library() and the A/B library work as they do with ctypes.  The GIL is held across the call: a queued launch
// makes no HIP call and returns in about 0.1 us, less than releasing the GIL costs.
// Stable ABI (Python 3.10 and later, where METH_FASTCALL belongs to it): one build loads into any later 3.x.
#define PY_SSIZE_T_CLEAN
#define Py_LIMITED_API 0x030A0000
#include <Python.h>

#include <stdint.h>
#include <string.h>

namespace {

typedef int (*plan_launch_fn)(void*, const void*, uint64_t, uint64_t, int, int);
typedef const char* (*last_error_fn)(void);
typedef uint64_t (*text_length_fn)(const void*);

struct TextBase {
    PyObject_HEAD
    PyObject* h;  // what `_h` reads: an int or None (owned)
    void* ptr;    // the same as a pointer, NULL for None
    uint64_t n;   // smartgpu_text_length(ptr) when h was set
    text_length_fn length;
};

struct PlanBase {
    PyObject_HEAD
    PyObject* h;
    void* ptr;
    plan_launch_fn launch;
    last_error_fn last_error;
};

PyTypeObject* g_text_type = nullptr;
PyObject* g_error = nullptr;  // engine.SmartGpuError (set_error_class)
PyObject *g_s_slot, *g_s_timed, *g_s_off, *g_s_n, *g_s_text;

// an int or None -> (object to keep, pointer); anything else: TypeError
int handle_from(PyObject* v, void** ptr)
{
    if (!v) { PyErr_SetString(PyExc_AttributeError, "_h cannot be deleted"); return -1; }
    if (v == Py_None) { *ptr = nullptr; return 0; }
    if (!PyLong_Check(v)) { PyErr_SetString(PyExc_TypeError, "_h is an int or None"); return -1; }
    const unsigned long long p = PyLong_AsUnsignedLongLong(v);  // (negative or beyond 64 bits: OverflowError)
    if (p == static_cast<unsigned long long>(-1) && PyErr_Occurred()) return -1;
    *ptr = reinterpret_cast<void*>(static_cast<uintptr_t>(p));
    return 0;
}
static_assert(sizeof(void*) == sizeof(unsigned long long), "handles are 64-bit pointers");

// *slot = v (a new reference), dropping what it held last: the slot never points at a freed object
void keep(PyObject** slot, PyObject* v)
{
    PyObject* old = *slot;
    Py_INCREF(v);
    *slot = v;
    Py_XDECREF(old);
}

void* addr_from(PyObject* v)
{
    if (v == Py_None) return nullptr;
    return PyLong_AsVoidPtr(v);  // (NULL with an error set for what is no int)
}

// a Python integer (or what __index__ makes one) as uint64: negative or beyond 64 bits raises OverflowError, never folds
int as_u64(PyObject* v, unsigned long long* out)
{
    if (PyLong_Check(v)) {
        *out = PyLong_AsUnsignedLongLong(v);
    } else {
        PyObject* i = PyNumber_Index(v);
        if (!i) return -1;
        *out = PyLong_AsUnsignedLongLong(i);
        Py_DECREF(i);
    }
    return (*out == static_cast<unsigned long long>(-1) && PyErr_Occurred()) ? -1 : 0;
}

PyObject* base_new(PyTypeObject* type, PyObject*, PyObject*)  // (the subclasses' __init__ take what they like)
{
    allocfunc alloc = reinterpret_cast<allocfunc>(PyType_GetSlot(type, Py_tp_alloc));
    return alloc(type, 0);  // zeroed: h == NULL reads as None
}

void base_free(PyObject* self)
{
    PyTypeObject* tp = Py_TYPE(self);
    reinterpret_cast<freefunc>(PyType_GetSlot(tp, Py_tp_free))(self);
    Py_DECREF(tp);  // (a heap type: its instances hold it)
}

// ---- TextBase ----------------------------------------------------------------------------------------------------------
void text_dealloc(PyObject* self)
{
    Py_XDECREF(reinterpret_cast<TextBase*>(self)->h);
    base_free(self);
}

PyObject* text_get_h(PyObject* self, void*)
{
    PyObject* h = reinterpret_cast<TextBase*>(self)->h;
    if (!h) h = Py_None;
    Py_INCREF(h);
    return h;
}

int text_set_h(PyObject* self, PyObject* v, void*)
{
    TextBase* t = reinterpret_cast<TextBase*>(self);
    void* p = nullptr;
    if (handle_from(v, &p) != 0) return -1;
    if (p && !t->length) { PyErr_SetString(PyExc_RuntimeError, "set a text's handle after _bind(), which says how its length is read"); return -1; }
    keep(&t->h, v);
    t->ptr = p;
    t->n = p ? t->length(p) : 0;
    return 0;
}

PyObject* text_bind(PyObject* self, PyObject* arg)  // _bind(address of smartgpu_text_length)
{
    void* f = addr_from(arg);
    if (!f && PyErr_Occurred()) return nullptr;
    reinterpret_cast<TextBase*>(self)->length = reinterpret_cast<text_length_fn>(f);
    Py_RETURN_NONE;
}

PyObject* text_length(PyObject* self, PyObject*)  // _length(): the length as it was read when the handle was set
{
    return PyLong_FromUnsignedLongLong(reinterpret_cast<TextBase*>(self)->n);
}

// ---- PlanBase ----------------------------------------------------------------------------------------------------------
void plan_dealloc(PyObject* self)
{
    Py_XDECREF(reinterpret_cast<PlanBase*>(self)->h);
    base_free(self);
}

PyObject* plan_get_h(PyObject* self, void*)
{
    PyObject* h = reinterpret_cast<PlanBase*>(self)->h;
    if (!h) h = Py_None;
    Py_INCREF(h);
    return h;
}

int plan_set_h(PyObject* self, PyObject* v, void*)
{
    PlanBase* p = reinterpret_cast<PlanBase*>(self);
    void* ptr = nullptr;
    if (handle_from(v, &ptr) != 0) return -1;
    keep(&p->h, v);
    p->ptr = ptr;
    return 0;
}

PyObject* plan_bind(PyObject* self, PyObject* args)  // _bind(address of smartgpu_plan_launch, of smartgpu_last_error)
{
    PyObject *a = nullptr, *b = nullptr;
    if (!PyArg_ParseTuple(args, "OO:_bind", &a, &b)) return nullptr;
    void* launch = addr_from(a);
    if (!launch && PyErr_Occurred()) return nullptr;
    void* err = addr_from(b);
    if (!err && PyErr_Occurred()) return nullptr;
    PlanBase* p = reinterpret_cast<PlanBase*>(self);
    p->launch = reinterpret_cast<plan_launch_fn>(launch);
    p->last_error = reinterpret_cast<last_error_fn>(err);
    Py_RETURN_NONE;
}

// launch(text, slot=0, timed=False, off=0, n=None)
PyObject* plan_launch(PyObject* self, PyObject* const* args, Py_ssize_t nargs, PyObject* kwnames)
{
    PlanBase* p = reinterpret_cast<PlanBase*>(self);
    PyObject* v[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // text, slot, timed, off, n (borrowed)
    if (nargs > 5) { PyErr_Format(PyExc_TypeError, "launch() takes at most 5 arguments (%zd given)", nargs); return nullptr; }
    for (Py_ssize_t i = 0; i < nargs; ++i) v[i] = args[i];
    if (kwnames) {
        PyObject* const names[5] = {g_s_text, g_s_slot, g_s_timed, g_s_off, g_s_n};
        const Py_ssize_t nkw = PyTuple_Size(kwnames);
        for (Py_ssize_t k = 0; k < nkw; ++k) {
            PyObject* name = PyTuple_GetItem(kwnames, k);
            int at = 0;
            while (at < 5 && name != names[at]) ++at;  // (keyword names of a call site are interned: mostly this hits)
            if (at == 5)
                for (at = 0; at < 5; ++at) {
                    const int eq = PyObject_RichCompareBool(name, names[at], Py_EQ);
                    if (eq < 0) return nullptr;
                    if (eq) break;
                }
            if (at == 5) { PyErr_Format(PyExc_TypeError, "launch() got an unexpected keyword argument '%U'", name); return nullptr; }
            if (v[at]) { PyErr_Format(PyExc_TypeError, "launch() got multiple values for argument '%U'", name); return nullptr; }
            v[at] = args[nargs + k];
        }
    }
    if (!v[0]) { PyErr_SetString(PyExc_TypeError, "launch() missing required argument 'text'"); return nullptr; }
    if (!PyObject_TypeCheck(v[0], g_text_type)) {
        PyErr_SetString(PyExc_TypeError, "launch() takes a Text");
        return nullptr;
    }
    const TextBase* t = reinterpret_cast<const TextBase*>(v[0]);
    long slot = 0;
    if (v[1]) {
        slot = PyLong_AsLong(v[1]);
        if (slot == -1 && PyErr_Occurred()) return nullptr;
        if (slot < INT32_MIN || slot > INT32_MAX) { PyErr_SetString(PyExc_OverflowError, "slot does not fit an int"); return nullptr; }
    }
    int timed = 0;
    if (v[2]) {
        timed = PyObject_IsTrue(v[2]);
        if (timed < 0) return nullptr;
    }
    unsigned long long off = 0;
    if (v[3] && as_u64(v[3], &off) != 0) return nullptr;
    unsigned long long n = 0;
    if (v[4] && v[4] != Py_None) {
        if (as_u64(v[4], &n) != 0) return nullptr;
    } else if (off <= t->n) {
        n = t->n - off;
    } else {
        PyErr_Format(PyExc_ValueError, "off %llu lies beyond the text (%llu bytes)", off, static_cast<unsigned long long>(t->n));
        return nullptr;
    }
    if (!p->launch || !p->last_error) { PyErr_SetString(PyExc_RuntimeError, "launch() before _bind()"); return nullptr; }
    if (p->launch(p->ptr, t->ptr, off, n, static_cast<int>(slot), timed) != 0) {
        const char* why = p->last_error();
        PyErr_Format(g_error ? g_error : PyExc_RuntimeError, "plan_launch: %s", why ? why : "");
        return nullptr;
    }
    Py_RETURN_NONE;
}

PyObject* set_error_class(PyObject*, PyObject* cls)
{
    keep(&g_error, cls);
    Py_RETURN_NONE;
}

PyGetSetDef text_getset[] = {
    {"_h", text_get_h, text_set_h, "the library's handle: an int, or None after free()", nullptr},
    {nullptr, nullptr, nullptr, nullptr, nullptr}};
PyMethodDef text_methods[] = {
    {"_bind", text_bind, METH_O, "_bind(address of smartgpu_text_length), before the handle is set"},
    {"_length", text_length, METH_NOARGS, "the text's length as read when the handle was set"},
    {nullptr, nullptr, 0, nullptr}};
PyType_Slot text_slots[] = {
    {Py_tp_new, reinterpret_cast<void*>(base_new)},
    {Py_tp_dealloc, reinterpret_cast<void*>(text_dealloc)},
    {Py_tp_getset, text_getset},
    {Py_tp_methods, text_methods},
    {0, nullptr}};
PyType_Spec text_spec = {"smart_amd._fastcall.TextBase", sizeof(TextBase), 0, Py_TPFLAGS_DEFAULT | Py_TPFLAGS_BASETYPE, text_slots};

PyGetSetDef plan_getset[] = {
    {"_h", plan_get_h, plan_set_h, "the library's handle: an int, or None after free()", nullptr},
    {nullptr, nullptr, nullptr, nullptr, nullptr}};
PyMethodDef plan_methods[] = {
    {"_bind", plan_bind, METH_VARARGS, "_bind(address of smartgpu_plan_launch, address of smartgpu_last_error)"},
    {"launch", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)(void)>(plan_launch)), METH_FASTCALL | METH_KEYWORDS,
     "launch(text, slot=0, timed=False, off=0, n=None): smartgpu_plan_launch over text[off..off+n), n=None to the end"},
    {nullptr, nullptr, 0, nullptr}};
PyType_Slot plan_slots[] = {
    {Py_tp_new, reinterpret_cast<void*>(base_new)},
    {Py_tp_dealloc, reinterpret_cast<void*>(plan_dealloc)},
    {Py_tp_getset, plan_getset},
    {Py_tp_methods, plan_methods},
    {0, nullptr}};
PyType_Spec plan_spec = {"smart_amd._fastcall.PlanBase", sizeof(PlanBase), 0, Py_TPFLAGS_DEFAULT | Py_TPFLAGS_BASETYPE, plan_slots};

PyMethodDef module_methods[] = {
    {"set_error_class", set_error_class, METH_O, "the exception a failed launch raises (engine.SmartGpuError)"},
    {nullptr, nullptr, 0, nullptr}};
PyModuleDef module_def = {PyModuleDef_HEAD_INIT, "_fastcall", "native Plan.launch (smart_amd/csrc/fastcall.cpp)", -1, module_methods,
                          nullptr, nullptr, nullptr, nullptr};

}  // namespace

PyMODINIT_FUNC PyInit__fastcall(void)
{
    PyObject* m = PyModule_Create(&module_def);
    if (!m) return nullptr;
    g_s_text = PyUnicode_InternFromString("text");
    g_s_slot = PyUnicode_InternFromString("slot");
    g_s_timed = PyUnicode_InternFromString("timed");
    g_s_off = PyUnicode_InternFromString("off");
    g_s_n = PyUnicode_InternFromString("n");
    PyObject* text = PyType_FromSpec(&text_spec);
    PyObject* plan = PyType_FromSpec(&plan_spec);
    if (!g_s_text || !g_s_slot || !g_s_timed || !g_s_off || !g_s_n || !text || !plan) { Py_DECREF(m); return nullptr; }
    g_text_type = reinterpret_cast<PyTypeObject*>(text);
    Py_INCREF(text);  // (g_text_type keeps one, the module the other)
    if (PyModule_AddObject(m, "TextBase", text) != 0 || PyModule_AddObject(m, "PlanBase", plan) != 0) { Py_DECREF(m); return nullptr; }
    return m;
}
